"""HiFi-GAN V1 generator on the MI355X contraction kernel.

Drop-in for `nntts.vocoders.hifigan_model.Generator` (nntts/vocoders/hifigan_model.py:95-150): same
constructor argument (the config object / dict of HiFiGAN_LJ_V1/config.json), same parameter names and
shapes (`state_dict` of the reference loads unchanged, weight_g / weight_v pairs), `forward(mel [B, 80, T])
-> audio [B, 1, T * prod(upsample_rates)]`, `remove_weight_norm()`.  Inference only.

Every Conv1d / ConvTranspose1d is one `efts_gemm` launch on channel-last rows (one row per sample):
  * dilated k = 3 / 7 / 11 convolutions: `taps`, `dilation` of the kernel (the tap offset is a row offset into
    the LDS window, exactly like the acoustic model's k5 convolutions);
  * the residual blocks are pre-activation (`conv(leaky(x))`, :45-52): the PRODUCER of x writes the operand
    plane of leaky(x) (`plane_act`), so no activation pass exists; `xt` between the two convolutions of a
    pair only ever lives as that plane (no fp32 copy);
  * ConvTranspose1d(stride u, kernel 2u, padding u/2) = a 2-tap convolution with u * cout output columns:
    y[n] = x[q] w[r] + x[q-1] w[r+u] with n + u/2 = q u + r; the [T+1][u*cout] result IS the [u(T+1)][cout] row
    space of the next stage (a pointer offset of u/2 rows);
  * the multi-receptive-field mean and the LeakyReLU of the next layer's input: `efts_mean_act_rows`;
  * conv_post + tanh: the kernel's tanh epilogue.
`resblock: "2"` (ResBlock2, hifigan_model.py:71-93; the V3 configuration): a block is two turns x <- x + conv_{k,d}(leaky(x)), d =
dilation[0], dilation[1].  Two ways to run one, chosen per block by `fused_resblock2`: ONE `efts_resblock2` launch
(csrc/efts_resblock2.hip: the intermediate and its operand plane stay in LDS; c <= 128, (k - 1) / 2 * (d0 + d1) <= 64 rows), or two
`efts_gemm` launches ((k - 1) * d <= 64 rows each).  V3's third block (k = 7, d = 12: a 72-row window) runs on the fused launch only.
The measured default composes where it can (tools/micro/vocoder_rb2_timing.py); what neither can run is refused in the constructor.
`resblock: "1"` generators issue exactly the launches they issued before.
Batches: the B utterances share one row space per stage, item b at rows b * P .. b * P + T_b * up with a pitch of
P = (T + gap) * up rows.  `gap` spare mel frames (`gap_frames`) come from the configuration: at the first upsampled
stage they are gap * upsample_rates[0] zero rows, and that must be no less than the largest halo of a residual
convolution, max (k - 1) / 2 * d; never fewer than 4 frames, which cover conv_pre (3 rows at mel rate) and the extra
input row of the transposed convolutions.  V1: max(4, ceil(25 / 8)) = 4 frames, 32 rows against a halo of
(11 - 1) / 2 * 5 = 25.  Every launch carries the per-row validity mask of its stage, so rows past an item's own
length stay zero exactly as the zero padding of a single-utterance run does; `forward(mel, lengths)` therefore equals
B separate calls on the unpadded items.
Configurations the launches below cannot compute are refused in the constructor (`_refusal`), never at a launch.
There is no CPU path.
"""
from __future__ import annotations

import contextlib
import ctypes
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


def _cfg(h, key, default=None):
    return h[key] if isinstance(h, dict) and key in h else getattr(h, key, default)


def gap_frames(upsample_rates, res_kernels, res_dilations) -> int:
    """spare mel frames between the items of a batch: their rows at the first upsampled stage hold the largest halo of a
    residual convolution (the later stages only have more rows per frame)"""
    halo = max((k - 1) // 2 * d for k, ds in zip(res_kernels, res_dilations) for d in ds)
    return max(_MIN_GAP_FRAMES, -(-halo // upsample_rates[0]))


def _rb2_fusable(c: int, k: int, ds) -> bool:
    """one efts_resblock2 launch can run this ResBlock2"""
    return c <= _RB2_MAX_C and k in _RB2_TAPS and (k - 1) // 2 * (ds[0] + ds[1]) <= _RB2_MAX_HALO


def _rb2_composable(k: int, ds) -> bool:
    """two efts_gemm launches can run this ResBlock2"""
    return k in _GEMM_TAPS and all((k - 1) * d <= _GEMM_MAX_SPAN for d in ds)


def _refusal(rates, kernels, res_kernels, res_dilations, c0, num_mels, resblock: str = "1") -> Optional[str]:
    """why the launches of `_run` cannot compute this configuration (None: they can)"""
    if resblock not in ("1", "2"):
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
        if resblock == "2" and len(ds) != 2:
            return (f"resblock '2' with {len(ds)} dilations for kernel size {k}: the reference's ResBlock2 uses exactly dilation[0] and "
                    "dilation[1] (a list of three is a ResBlock1 configuration)")
        for d in ds:
            if d < 1 or (resblock == "1" and (k - 1) * d > _GEMM_MAX_SPAN):
                return f"residual kernel size {k} with dilation {d}: efts_gemm takes (k - 1) * d <= {_GEMM_MAX_SPAN} rows, d >= 1"
        if resblock == "2" and not _rb2_composable(k, ds):
            # a window span above 64 rows: only the fused launch can run it, in every stage
            c_max = c0 // 2 if c0 > 0 else 0
            if c_max > _RB2_MAX_C:
                return (f"ResBlock2 with kernel size {k} and dilations {list(ds)} at {c_max} channels: (k - 1) * d above {_GEMM_MAX_SPAN} rows "
                        f"is beyond efts_gemm, and efts_resblock2 takes c <= {_RB2_MAX_C}")
            if k not in _RB2_TAPS or (k - 1) // 2 * (ds[0] + ds[1]) > _RB2_MAX_HALO:
                return (f"ResBlock2 with kernel size {k} and dilations {list(ds)}: (k - 1) * d above {_GEMM_MAX_SPAN} rows is beyond efts_gemm, "
                        f"and efts_resblock2 takes (k - 1) / 2 * (d0 + d1) <= {_RB2_MAX_HALO} rows")
    c_last = c0 // 2 ** len(rates)
    if c0 <= 0 or c0 % 2 ** len(rates) or c_last % 4:
        return (f"upsample_initial_channel {c0} over {len(rates)} stages: every stage needs a whole channel count that is a multiple "
                "of 4 (the 4-column accesses of the elementwise kernels)")
    if not 1 <= num_mels <= 4096:
        return "num_mels must be in 1 .. 4096 (efts_pack_rows)"
    return None


class _ResBlock1(nn.Module):
    """parameter container with the reference's names (hifigan_model.py:30-43); never called"""

    def __init__(self, channels: int, kernel_size: int, dilation):
        super().__init__()
        pad = lambda d: (kernel_size * d - d) // 2
        self.convs1 = nn.ModuleList([weight_norm(nn.Conv1d(channels, channels, kernel_size, 1, dilation=d, padding=pad(d)))
                                     for d in dilation])
        self.convs2 = nn.ModuleList([weight_norm(nn.Conv1d(channels, channels, kernel_size, 1, dilation=1, padding=pad(1)))
                                     for _ in dilation])
        self.kernel_size, self.dilation = kernel_size, tuple(dilation)


class _ResBlock2(nn.Module):
    """parameter container with the reference's names (hifigan_model.py:71-79); never called"""

    def __init__(self, channels: int, kernel_size: int, dilation):
        super().__init__()
        pad = lambda d: (kernel_size * d - d) // 2
        self.convs = nn.ModuleList([weight_norm(nn.Conv1d(channels, channels, kernel_size, 1, dilation=d, padding=pad(d)))
                                    for d in dilation[:2]])
        self.kernel_size, self.dilation = kernel_size, tuple(dilation[:2])


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
        why = _refusal(self.upsample_rates, self.upsample_kernel_sizes, self.res_kernels, self.res_dilations, c0, self.num_mels,
                       self.resblock)
        if why is not None:
            raise NotImplementedError(why)
        self.gap_frames = gap_frames(self.upsample_rates, self.res_kernels, self.res_dilations)
        self.conv_pre = weight_norm(nn.Conv1d(self.num_mels, c0, 7, 1, padding=3))
        self.ups = nn.ModuleList([weight_norm(nn.ConvTranspose1d(c0 // 2 ** i, c0 // 2 ** (i + 1), k, u, padding=(k - u) // 2))
                                  for i, (u, k) in enumerate(zip(self.upsample_rates, self.upsample_kernel_sizes))])
        self.resblocks = nn.ModuleList()
        ch = c0
        for i in range(len(self.ups)):
            ch = c0 // 2 ** (i + 1)
            for k, d in zip(self.res_kernels, self.res_dilations):
                self.resblocks.append((_ResBlock2 if self.resblock == "2" else _ResBlock1)(ch, k, d))
        self.conv_post = weight_norm(nn.Conv1d(ch, 1, 7, 1, padding=3))
        self._packed: Optional[Dict[str, PackedWeight]] = None
        self._packed_dev = None
        self._bias: Dict[str, torch.Tensor] = {}
        self._bufs = Cache(capacity=3)          # (B, T) -> workspace
        # per-shape hipGraph of the ~85 launches of a call (round 6; efficient_tts_amd/graphs.py, the acoustic model's cache): one utterance is
        # 2 ms of device work issued by a host that needs about as long for the launches; `graphs = False`: every launch issued eagerly
        self.graphs = True
        # resblock "2": True = every ResBlock2 that efts_resblock2 can run is ONE launch (the intermediate stays in LDS) and two efts_gemm
        # launches run the others (more than 128 channels); False = two efts_gemm launches wherever they can run (window spans up to 64
        # rows) and the fused launch for the rest.  Measured (tools/micro/vocoder_rb2_timing.py, profiles/vocoder_rb2_timing.json): V3 at one
        # 800-frame utterance 0.87 ms fused against 0.74 ms composed, 4.79 against 3.95 ms at a batch of 8 -- so the default composes and the
        # fused launch runs the blocks only it can run (V3: k = 7, d = 12)
        self.fused_resblock2 = False
        self.branch_streams = True          # the residual blocks of a stage on streams of their own (False: one after the other, A/B)
        from .graphs import GraphCache
        object.__setattr__(self, "_graph_cache", GraphCache(capacity=4))

    # ------------------------------------------------------------------ reference API
    def remove_weight_norm(self):
        self._graph_cache.clear()
        for m in [self.conv_pre, self.conv_post, *self.ups]:
            remove_weight_norm(m)
        for rb in self.resblocks:
            for m in ([*rb.convs] if self.resblock == "2" else [*rb.convs1, *rb.convs2]):
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

    def _pack(self, dev) -> Dict[str, PackedWeight]:
        if self._packed is not None and self._packed_dev == dev:
            return self._packed
        self._bufs.clear()                      # workspaces of another device are of no use either
        self._packed_dev = dev
        pk: Dict[str, PackedWeight] = {}
        with O.stream_scope():
            def conv(name, m):
                w = self._folded(m).float().contiguous()
                pk[name] = PackedWeight(w.shape[0], w.shape[1], w.shape[2], self.split, dev)
                pk[name].pack(w)
                self._bias[name] = m.bias.detach().float().contiguous()

            conv("conv_pre", self.conv_pre)
            conv("conv_post", self.conv_post)
            for i, (m, u) in enumerate(zip(self.ups, self.upsample_rates)):
                w = self._folded(m).float()                                  # [cin][cout][2u]
                cin, cout, _ = w.shape
                # B[tap][n = r * cout + co][ci]: tap 0 multiplies x[q-1] (w[.., r + u]), tap 1 multiplies x[q] (w[.., r]), tap 2 = 0
                b = torch.zeros(u * cout, cin, 3, device=dev)
                b[:, :, 0] = w[:, :, u:].permute(2, 1, 0).reshape(u * cout, cin)
                b[:, :, 1] = w[:, :, :u].permute(2, 1, 0).reshape(u * cout, cin)
                pk[f"ups.{i}"] = PackedWeight(u * cout, cin, 3, self.split, dev)
                pk[f"ups.{i}"].pack(b.contiguous())
                self._bias[f"ups.{i}"] = m.bias.detach().float().repeat(u).contiguous()
            for n, rb in enumerate(self.resblocks):
                for d in range(len(rb.dilation)):
                    if self.resblock == "2":
                        conv(f"rb{n}.c.{d}", rb.convs[d])
                        continue
                    conv(f"rb{n}.c1.{d}", rb.convs1[d])
                    conv(f"rb{n}.c2.{d}", rb.convs2[d])
        self._packed = pk
        return pk

    # ------------------------------------------------------------------ buffers per mel length
    def _workspace_for(self, B: int, T: int, dev) -> dict:
        return self._bufs.get((B, T), lambda: self._make_workspace(B, T, dev))

    def _make_workspace(self, B: int, T: int, dev) -> dict:
        sp = self.split
        pitch = T + self.gap_frames                                            # rows per item at mel rate
        rows = B * pitch
        b = {"pitch": pitch, "mel": _Rows(rows, self.num_mels, sp, dev, f32=False),
             "pre": _Rows(rows, self.conv_pre.out_channels, sp, dev, f32=False), "mask": []}
        for i, (m, u) in enumerate(zip(self.ups, self.upsample_rates)):
            cout = m.out_channels
            n_i = rows * u
            b[f"up{i}"] = _Rows((rows + 1) * u, cout, sp, dev, plane=False)  # the [rows + 1][u * cout] GEMM result, seen as rows of cout
            b[f"x{i}"] = _Rows(n_i, cout, sp, dev, f32=False)                # plane of leaky(x_i)
            if self.resblock == "1":
                b[f"t{i}"] = [_Rows(n_i, cout, sp, dev, f32=False) for _ in self.res_kernels]   # plane of leaky(xt), one per residual block (they run side by side)
            b[f"r{i}"] = [[_Rows(n_i, cout, sp, dev) for _ in range(2)] for _ in self.res_kernels]   # ping-pong per residual block
            b[f"s{i}"] = _Rows(n_i, cout, sp, dev, f32=False)                # plane of leaky(mean)
            b["mask"].append(torch.zeros(n_i + 1, dtype=torch.float32, device=dev))
            rows = n_i
        b["mask_mel"] = torch.zeros(B * pitch + 1, dtype=torch.float32, device=dev)
        b["out"] = torch.zeros(rows + 256, 1, dtype=torch.float32, device=dev)
        return b

    def _branch_streams(self, dev, count: int):
        st = getattr(self, "_bstreams", None)
        if st is None or len(st) != count or (count and st[0].device != dev):
            st = [torch.cuda.Stream(device=dev) for _ in range(count)]
            object.__setattr__(self, "_bstreams", st)
        return st

    # ------------------------------------------------------------------ forward
    @torch.no_grad()
    def forward(self, x: torch.Tensor, lengths: Optional[torch.Tensor] = None, keep: Optional[dict] = None) -> torch.Tensor:
        """mel [B, num_mels, T] -> audio [B, 1, T * hop].  `lengths` (frames per item, optional): every item is
        synthesised exactly as if it had been passed alone without its padding; samples past lengths[b] * hop are 0.
        `keep` (a dict, for the tests; like `_forward_impl(..., keep=True)` of the acoustic model): every step's output buffer is
        cloned into it (`_run`), which works with eagerly issued launches only: `graphs = False`, never under capture."""
        if x.dim() != 3 or x.shape[1] != self.num_mels:
            raise ValueError(f"expected mel [B, {self.num_mels}, T]")
        if not x.is_cuda:
            raise RuntimeError("HiFiGANGenerator runs on an MI355X device only (no CPU path)")
        L.load()
        L.require_device()
        dev = x.device
        pk = self._pack(dev)
        B, _, T = x.shape
        hop = 1
        for u in self.upsample_rates:
            hop *= u
        if lengths is None:
            lens = torch.full((B,), T, dtype=torch.int32, device=dev)
        else:
            lens = lengths.to(device=dev, dtype=torch.int32).clamp(0, T)
        mel = x.transpose(1, 2).float()
        if lengths is not None:                 # what the padding frames hold must not reach conv_pre's halo
            mel = mel * (torch.arange(T, device=dev)[None, :] < lens[:, None])[:, :, None]
        mel = mel.contiguous()

        def body(mel_btc, lens_i32):
            audio = torch.zeros(B, 1, T * hop, dtype=torch.float32, device=dev)
            with O.stream_scope():
                self._run(pk, mel_btc, lens_i32, audio, B, T, hop, dev, keep)
            return (audio,)

        if keep is not None and (self.graphs or torch.cuda.is_current_stream_capturing()):
            raise RuntimeError("keep: the stages are observed on eagerly issued launches only (graphs = False, no capture)")
        if not self.graphs or torch.cuda.is_current_stream_capturing():
            return body(mel, lens)[0]
        ws = self._workspace_for(B, T, dev)
        # the graph is valid while the buffers its launches point at live: this workspace and the packed planes
        tag = (id(ws), tuple(w.ptr for w in pk.values()), self.split, self.fused_resblock2)
        return self._graph_cache.run(("voc", B, T), tag, (mel, lens), body, keepalive=(ws, pk), adaptive=True)[0]

    def _conv(self, pk, name, a: Plane, rows, taps, dil, *, mask=None, out_f=None, ldo=0, out_p=None, plane_slope=None, resid=None,
              ldr=0, act=L.ACT_NONE):
        w = pk[name]
        O.gemm(a=a, b_ptr=w.ptr, ldb=w.ld, b_tap_stride=w.tap_stride, taps=taps, m=rows, n=w.cout, bias=self._bias[name], act=act,
               resid_ptr=resid, ldr=ldr, rowmask_ptr=None if mask is None else mask.data_ptr(), out_f32_ptr=out_f, ldo=ldo,
               out_plane=out_p, dilation=dil, plane_act=plane_slope is not None, plane_slope=0.0 if plane_slope is None else plane_slope)

    def _rb2_fused(self, c: int, k: int, ds) -> bool:
        """which launches run a ResBlock2 of this geometry (`fused_resblock2`; the constructor refused what neither can)"""
        if self.fused_resblock2:
            return _rb2_fusable(c, k, ds)
        return not _rb2_composable(k, ds)

    def _resblock2(self, pk, n: int, x_f: int, x_p: Plane, pp, rows: int, c: int, k: int, ds, mask: torch.Tensor) -> int:
        """ResBlock2 n (hifigan_model.py:81-88) on the current stream: x <- x + conv_{k,d}(leaky(x)) for d = ds[0], ds[1]; returns the
        pointer of the fp32 result (pp[1])"""
        if self._rb2_fused(c, k, ds):
            w0, w1 = pk[f"rb{n}.c.0"], pk[f"rb{n}.c.1"]
            g = L.ResBlock2Args()
            g.x, g.ldx, g.p0, g.ldp = x_f, c, x_p.ptr, x_p.ld
            g.w0, g.w1, g.ldw, g.w_tap_stride = w0.ptr, w1.ptr, w0.ld, w0.tap_stride
            g.bias0, g.bias1 = self._bias[f"rb{n}.c.0"].data_ptr(), self._bias[f"rb{n}.c.1"].data_ptr()
            g.rowmask, g.out, g.ldo = mask.data_ptr(), pp[1].fptr, c
            g.split, g.m, g.c, g.k, g.d0, g.d1, g.slope = self.split, rows, c, k, ds[0], ds[1], LRELU_SLOPE
            L.check(L.load().efts_resblock2(ctypes.byref(g), O._stream()), "efts_resblock2")
            return pp[1].fptr
        # one efts_gemm launch per turn: the first also writes the operand plane of leaky(y1) for the second
        self._conv(pk, f"rb{n}.c.0", x_p, rows, k, ds[0], mask=mask, out_f=pp[0].fptr, ldo=c, out_p=pp[0].p, plane_slope=LRELU_SLOPE,
                   resid=x_f, ldr=c)
        self._conv(pk, f"rb{n}.c.1", pp[0].p, rows, k, ds[1], mask=mask, out_f=pp[1].fptr, ldo=c, resid=pp[0].fptr, ldr=c)
        return pp[1].fptr

    def _run(self, pk, mel_btc: torch.Tensor, lens: torch.Tensor, audio: torch.Tensor, B: int, T: int, hop: int, dev,
             keep: Optional[dict] = None) -> None:
        """keep (None: nothing happens): after each step a clone of what it wrote, made on the stream of the step's launch and complete
        when `_run` returns (it ends with a device synchronisation then).  Whole buffers, guard rows included: "pre", "x{i}", "s{i}"
        operand planes (uint8 [alloc][ld], row 0 at _GUARD); "r{i}.{j}.{d}" fp32 [alloc][c] of residual block j after pair d (resblock "2":
        "r{i}.{j}", the block's fp32 output);
        "up{i}" fp32 [rows][c] behind the u / 2-row offset; "out" fp32 [rows + 256][1]; "pitch": rows per item at mel rate."""
        b = self._workspace_for(B, T, dev)
        lib = L.load()
        sp = self.split
        pitch = b["pitch"]
        st = O._stream()

        def masks(into: torch.Tensor, lengths_i32: torch.Tensor, t_max: int, t_pitch: int):
            L.check(lib.efts_row_masks(lengths_i32.data_ptr(), None, into.data_ptr(), B, t_max, t_pitch, st), "efts_row_masks")

        mel_p = b["mel"].p
        L.check(lib.efts_pack_rows(mel_btc.data_ptr(), None, mel_p.ptr, mel_p.ld, B, T, pitch, self.num_mels,
                                   mel_p.nchunk * O.chunk_k(sp), sp, st), "efts_pack_rows")
        masks(b["mask_mel"], lens, T, pitch)
        # conv_pre (:118); its only consumer applies leaky first (:120) -> the plane of leaky(x), no fp32 copy
        rows = B * pitch
        self._conv(pk, "conv_pre", mel_p, rows, 7, 1, mask=b["mask_mel"], out_p=b["pre"].p, plane_slope=LRELU_SLOPE)
        if keep is not None:
            keep["pitch"], keep["pre"] = pitch, b["pre"].p.buf.clone()
        cur_p, n, up_total = b["pre"].p, 0, 1
        for i, u in enumerate(self.upsample_rates):
            cout = self.ups[i].out_channels
            up_total *= u
            n_i = rows * u
            mask = b["mask"][i]
            masks(mask, lens * up_total, T * up_total, pitch * up_total)
            up = b[f"up{i}"]
            # ConvTranspose1d as a 2-tap convolution over the input rows + 1 (the row after the last one is a zero guard row)
            self._conv(pk, f"ups.{i}", cur_p, rows + 1, 3, 1, out_f=up.fptr, ldo=u * cout)
            x_f = up.fptr + (u // 2) * cout * 4                               # y[n] = row n + u/2 of the flattened result
            x_p = b[f"x{i}"].p
            # plane of leaky(x): x * (x > 0 ? 1 : slope), the identity-residual LeakyReLU mode of efts_act_bwd; the mask drops
            # the transposed convolution's cropped border samples, which land in the zero rows between items
            L.check(lib.efts_act_bwd(x_f, x_f, None, mask.data_ptr(), LRELU_SLOPE, 3, None, x_p.ptr, x_p.ld, sp, None, n_i, cout, st),
                    "efts_act_bwd")
            if keep is not None:
                lo = (_GUARD + u // 2) * cout
                keep[f"up{i}"], keep[f"x{i}"] = up.f.view(-1)[lo:lo + n_i * cout].view(n_i, cout).clone(), x_p.buf.clone()
            # The residual blocks of a stage (kernel sizes 3 / 7 / 11) are independent until their mean (:123-128): each runs as a chain of its own
            # on its own stream (round 6).  At one utterance a launch is 50-200 workgroups for 15-30 us: eighteen of them in a row per stage were
            # latency, not work (profiles/rocprofv3_r06_vocoder_summary.txt); two chains' workgroups fit a CU's LDS side by side.
            finals: List[int] = [0] * len(self.res_kernels)
            main = torch.cuda.current_stream(dev)
            side = self._branch_streams(dev, len(self.res_kernels) - 1) if self.branch_streams else []
            ev_x = torch.cuda.Event()
            ev_x.record(main)
            joins = []
            order = sorted(range(len(self.res_kernels)), key=lambda j: -self.res_kernels[j])       # the longest chain is issued first
            for slot, j in enumerate(order):
                k = self.res_kernels[j]
                rb = self.resblocks[n + j]
                own = side[slot] if slot < len(side) else None                                   # the last (shortest) chain stays on the main stream
                if own is not None:
                    own.wait_event(ev_x)
                with (O.on_stream(own) if own is not None else contextlib.nullcontext()):
                    r_f, r_p, pp = x_f, x_p, b[f"r{i}"][j]
                    if self.resblock == "2":
                        r_f = self._resblock2(pk, n + j, x_f, x_p, pp, n_i, cout, k, rb.dilation, mask)
                        if keep is not None:
                            keep[f"r{i}.{j}"] = pp[1].f.clone()
                    tp = b[f"t{i}"][j].p if self.resblock == "1" else None
                    for d_i, d in enumerate(rb.dilation if self.resblock == "1" else ()):
                        self._conv(pk, f"rb{n + j}.c1.{d_i}", r_p, n_i, k, d, mask=mask, out_p=tp, plane_slope=LRELU_SLOPE)  # :47-48 (+ :49)
                        nxt = pp[d_i & 1]
                        self._conv(pk, f"rb{n + j}.c2.{d_i}", tp, n_i, k, 1, mask=mask, out_f=nxt.fptr, ldo=cout, out_p=nxt.p,
                                   plane_slope=LRELU_SLOPE, resid=r_f, ldr=cout)                                        # :50-51
                        r_f, r_p = nxt.fptr, nxt.p
                        if keep is not None:            # (on this chain's stream: the next pair but one writes this buffer again)
                            keep[f"r{i}.{j}.{d_i}"] = nxt.f.clone()
                    finals[j] = r_f
                    if own is not None:
                        ev = torch.cuda.Event()
                        ev.record(own)
                        joins.append(ev)
            for ev in joins:
                main.wait_event(ev)
            n += len(self.res_kernels)
            last = i == len(self.upsample_rates) - 1
            s_p = b[f"s{i}"].p
            L.check(lib.efts_mean_act_rows(finals[0], finals[1] if len(finals) > 1 else None, finals[2] if len(finals) > 2 else None,
                                           cout, 1.0 / len(finals), 0.01 if last else LRELU_SLOPE, None, 0, s_p.ptr, s_p.ld, sp, n_i, cout,
                                           st), "efts_mean_act_rows")                                              # :128 (+ :120 / :129)
            if keep is not None:
                keep[f"s{i}"] = s_p.buf.clone()
            cur_p, rows = s_p, n_i
        self._conv(pk, "conv_post", cur_p, rows, 7, 1, mask=b["mask"][-1], out_f=b["out"].data_ptr(), ldo=1, act=L.ACT_TANH)   # :130-131
        audio[:, 0].copy_(b["out"][:rows, 0].view(B, pitch * hop)[:, :T * hop])
        if keep is not None:
            keep["out"] = b["out"].clone()
            torch.cuda.synchronize(dev)                 # the side streams' clones included


def load_hifigan_generator(device, config_path: str, checkpoint_path: str, precision: str = "bf16x3") -> HiFiGANGenerator:
    """The reference's loader (hifigan_model.py:18-28) with explicit paths: JSON config + a checkpoint whose
    "generator" entry is the reference Generator's state_dict (the published `generator_v1` is not shipped with the
    reference repository)."""
    import json
    with open(config_path) as f:
        cfg = json.load(f)
    gen = HiFiGANGenerator(cfg, precision=precision)
    state = torch.load(checkpoint_path, map_location="cpu")
    gen.load_state_dict(state["generator"] if "generator" in state else state)
    gen = gen.to(device).eval()
    gen.remove_weight_norm()
    return gen
