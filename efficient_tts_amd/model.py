"""EfficientTTSCNN on MI355X: the host-side mirror of the reference model class.

Same class name, ctor kwargs, ``forward`` / ``inference`` signatures and returns, and
``state_dict`` keys as ``nntts.models.EfficientTTSCNN`` (reference
nntts/models/efficient_tts.py:23-418), so ``getattr(pkg.models, config["model_name"])(**config["model_params"])``
(nntts/bin/train.py:173-185) and reference checkpoints work unchanged.  All arithmetic runs in
hand-written HIP kernels behind the C ABI of ``libefts_hip.so`` (include/efts_abi.h); PyTorch
only owns device memory, streams and the parameter containers.  There is no torch/CPU
fallback: without the library or a gfx950 device the model raises.
"""
from __future__ import annotations

import dataclasses
import os
import logging
from collections import namedtuple
from typing import Dict, Optional, Tuple

import torch

from . import lib as L
from . import ops as O
from .dropout import LAUNCH, NONE, DropoutPlan, dist_rank, rank_base
from .graphs import GraphCache, PadTo
from .ops import F32Rows, Plane, Rows, roundup
from .weights import WeightPlanes


# --------------------------------------------------------------------------------------
# Parameter containers.  torch.nn modules are used ONLY to hold/initialise parameters
# with the reference's names and default init order; their forward() is never called.
# --------------------------------------------------------------------------------------
class _ResConv1d(torch.nn.Module):                     # efts_modules.py:19-51 (names only)
    def __init__(self, n_channels, k_size, act, act_params, dropout_rate):
        super().__init__()
        mods = [torch.nn.Conv1d(n_channels, n_channels, kernel_size=k_size, padding=(k_size - 1) // 2),
                getattr(torch.nn, act)(**act_params)]
        if dropout_rate >= 1e-5:
            mods.append(torch.nn.Dropout(dropout_rate))
        self.conv = torch.nn.Sequential(*mods)


class _ResConvBlock(torch.nn.Module):                  # efts_modules.py:54-99 (names only)
    def __init__(self, num_layers, n_channels, k_size, act, act_params, dropout_rate, use_weight_norm):
        super().__init__()
        self.num_layers = num_layers
        self.layers = torch.nn.Sequential(*[_ResConv1d(n_channels, k_size, act, act_params, dropout_rate)
                                            for _ in range(num_layers)])
        if use_weight_norm:
            for m in self.modules():
                if isinstance(m, torch.nn.Conv1d):
                    torch.nn.utils.weight_norm(m)


class _DurationPredictor(torch.nn.Module):             # duration_predictor.py:28-64 (names only)
    def __init__(self, idim, n_layers, n_chans, kernel_size=3, dropout_rate=0.1, offset=1.0):
        super().__init__()
        self.offset, self.n_layers = offset, n_layers
        self.conv = torch.nn.ModuleList()
        for _ in range(n_layers):
            self.conv.append(torch.nn.Sequential(
                torch.nn.Conv1d(n_chans, n_chans, kernel_size, stride=1, padding=(kernel_size - 1) // 2),
                torch.nn.ReLU(),
                torch.nn.LayerNorm(n_chans, eps=1e-12),       # layer_norm.py:14-17
                torch.nn.Dropout(dropout_rate)))
        self.linear = torch.nn.Linear(n_chans, 1)


class LazyStats(dict):
    """``stats`` of the reference forward (efficient_tts.py:225-227) without the three
    per-step host syncs: values stay on the device until a key is read."""

    def __init__(self, out3: torch.Tensor):
        super().__init__(loss=None, mel_loss=None, duration_loss=None)
        self._t, self._v = out3, None

    def _vals(self):
        if self._v is None:
            self._v = self._t.tolist()
        return dict(loss=self._v[0], mel_loss=self._v[1], duration_loss=self._v[2])

    def __getitem__(self, k):
        return self._vals()[k]

    def get(self, k, default=None):
        return self._vals().get(k, default)

    def __iter__(self):
        return iter(("loss", "mel_loss", "duration_loss"))

    def keys(self):
        return self._vals().keys()

    def items(self):
        return self._vals().items()

    def values(self):
        return self._vals().values()

    def __repr__(self):
        return repr(self._vals())


class _Workspace:
    """Named device buffers for one (B, T1, T2) shape; zero-initialised once, so guard and gap
    rows stay zero (kernels never write them with non-zero values)."""

    _serial = 0

    def __init__(self, device):
        self.device = device
        self.bufs: Dict[str, object] = {}
        _Workspace._serial += 1
        self.serial = _Workspace._serial          # identifies the allocation: captured graphs point into these buffers

    def f32(self, name: str, rs: Rows, c: int) -> F32Rows:
        key = ("f", name, rs.B, rs.T, c)
        if key not in self.bufs:
            self.bufs[key] = F32Rows(rs, c, self.device)
        return self.bufs[key]

    def plane(self, name: str, rs: Rows, k: int, split: int) -> Plane:
        key = ("p", name, rs.B, rs.T, k, split)
        if key not in self.bufs:
            self.bufs[key] = Plane.for_rows(rs, k, split, self.device)
        return self.bufs[key]

    def raw_plane(self, name: str, nrows: int, k: int, split: int) -> Plane:
        key = ("rp", name, nrows, k, split)
        if key not in self.bufs:
            self.bufs[key] = Plane(nrows, k, split, self.device)
        return self.bufs[key]

    def get(self, key, make):
        """generic cached object (e.g. transposed planes of the training step)"""
        if key not in self.bufs:
            self.bufs[key] = make()
        return self.bufs[key]

    def tensor(self, name: str, shape, dtype=torch.float32) -> torch.Tensor:
        key = ("t", name, tuple(shape), dtype)
        if key not in self.bufs:
            self.bufs[key] = torch.zeros(*shape, dtype=dtype, device=self.device)
        return self.bufs[key]


PRECISIONS = {"bf16": 1, "bf16x3": 2, "fp32": 3}
TRAINABLE_PRECISIONS = ("bf16", "bf16x3")      # fp32 (operand format 3) is an eval-path mode: no backward, wgrad or optimiser form
# launch options whose fused kernels have no fp32 form: an fp32 model runs their generic fallback (efts_gemm on format-3 planes)
FP32_GENERIC_OPTIONS = ("resconv", "fuse_prenet", "fuse_expand", "embed_conv", "small_m")


def require_trainable(model, what: str) -> None:
    """NotImplementedError unless `model` (or the module a wrapper holds) runs in a precision the training path implements"""
    m = getattr(model, "module", model)
    prec = getattr(m, "precision", None)
    if prec is not None and prec not in TRAINABLE_PRECISIONS:
        raise NotImplementedError(f"{what}: training is implemented for precision {' / '.join(map(repr, TRAINABLE_PRECISIONS))}, "
                                  f"not {prec!r} (an inference / validation mode)")


@dataclasses.dataclass
class LaunchOptions:
    """Everything that changes WHICH launches a pass consists of (not their results): the A/B and test hooks of the model.  One object,
    so that the tags of the captured graphs are derived from it (`tag()`) instead of being enumerated by hand at every capture site
    -- an option that is missing from a tag replays a graph captured under the other setting.  Every field is also readable / writable
    as an attribute of the model (`model.resconv = False`); the finished A/Bs of earlier rounds (text layers as riders of the
    mel-encoder launches, CU halves for the prenet, duration-predictor riders) are no longer options: their winners are the code."""
    resconv: bool = True            # long row spaces: residual stacks on efts_resconv5 (False: efts_gemm + fp32 stream)
    resconv_min_rows: int = 16384   # ... from this many rows on (shorter ones keep the fp32 stream + efts_gemm, whose 124-row tiles fill the chip better)
    side_stream: bool = True        # text-length work on a second HIP stream beside the mel-length kernels
    fuse_prenet: bool = True        # the prenet straight from the fp32 frames (efts_frame_linear); False: efts_pack_rows + efts_gemm
    fuse_soft_index: bool = True    # T1 <= 128: q.k^T, softmax and soft index in one launch (False: scores stored, efts_attn_soft_index)
    fuse_align: bool = True         # imv scan + aligned positions + duration target in one launch (efts_imv_align)
    fuse_expand: bool = True        # T1 <= 256: alpha' generated in registers inside the expand contraction (efts_expand)
    fuse_mel_loss: bool = True      # the loss's mel term in the epilogue of the mel head's launch (efts_gemm_args.sqerr_part) where that launch fills the chip
    fuse_mel_loss_min_wgs: int = 0  # ... i.e. from this many 128-row tiles on (0: the number of CUs; tests lower it)
    embed_conv: bool = True         # eval paths: embedding + text-encoder layer 0 as table look-ups (efts_embed_conv)
    small_m: bool = True            # free-running inference on short row spaces: the K-split small-M tiling of efts_gemm
    small_m_rows: int = 1024        # ... up to this many rows

    def tag(self) -> tuple:
        return dataclasses.astuple(self) + (O.RC_KERNEL, O.GEMM_TILING)       # (the launch-level switches of ops.py change the launches too)


def lengths_and_masks(text_lengths, speech_lengths, dev, rs1: Rows, rs2: Rows, gap1, len1, gap2, len2):
    """The lengths as int32 device tensors and, where ONE launch can do it, the row masks of both row spaces (efficient_tts.py:137-139)
    -> (tl, ml, masks_done).  masks_done False (lengths of two dtypes, or not contiguous): only the two casts are enqueued, and the
    caller launches efts_row_masks per row space where its schedule wants them"""
    tl_d, ml_d = text_lengths.to(dev), speech_lengths.to(dev)
    if tl_d.dtype == ml_d.dtype and tl_d.dtype in (torch.int64, torch.int32) and tl_d.is_contiguous() and ml_d.is_contiguous():
        # both masks + the int32 copies of the lengths in one launch (two casts + two mask launches before)
        return (*O.row_masks_pair(tl_d, ml_d, rs1, rs2, gap1, len1, gap2, len2), True)
    return tl_d.to(torch.int32), ml_d.to(torch.int32), False


class _Pass:
    """What every stage of one teacher-forced forward reads.  ws: the workspace of the shape; pk: packed planes by layer name;
    rs1 / rs2: text- and mel-length row spaces; gap* / len*: their row masks (0 on the gap rows / beyond each item's length as well);
    tl / ml: int32 lengths on the device; main / side: the streams of the mel-length and the text-length work (main itself without
    side_stream); vt: the V^T plane of an unfused expand, else None; masks_done: gap1 / len1 are already enqueued (else only
    gap2 / len2 are, and the schedule launches the text masks behind the fork); drop: the pass's Dropout masks (dropout.DropoutPlan)"""
    __slots__ = ("ws", "pk", "text", "speech", "B", "T1", "T2", "rs1", "rs2", "gap1", "len1", "gap2", "len2", "tl", "ml", "main", "side",
                 "vt", "masks_done", "drop")

    def __init__(self, **fields):
        for k, v in fields.items():
            setattr(self, k, v)


# What a stage of the forward hands to the stages behind it (`_f`: F32Rows, `_p`: operand Plane, `_l`: lo plane of a split-1 stream).
_Embedded = namedtuple("_Embedded", "x_f x_p start")              # start: the first text-encoder layer still to run
_TextSide = namedtuple("_TextSide", "key_p val_f val_p")
_Prenet = namedtuple("_Prenet", "pre_f pre_p pre_l")
_Front = namedtuple("_Front", "q_p key_p val_f dur v_ready")      # val_f, dur, v_ready: None where an alignment-only pass skips them
_Aligned = namedtuple("_Aligned", "sidx imv e lde alpha")         # alpha: only for keep=True
_Head = namedtuple("_Head", "mel sqerr_part n_part")              # sqerr_part: the squared-error partials the head's epilogue left, or None


class _TextCursor:
    """The next text-encoder layer's efts_resconv5 keyword set: where the text stack stands while its layers are launched one by one
    (by themselves, or as riders of the mel-encoder launches).  x_p is the last launched layer's operand plane."""
    __slots__ = ("m", "st", "i", "ride_from", "x_f", "x_p", "x_lo")

    def __init__(self, model, st: _Pass, emb: _Embedded, ride_from: int):
        self.m, self.st, self.i, self.ride_from = model, st, emb.start, ride_from
        self.x_f, self.x_p, self.x_lo = emb.x_f, emb.x_p, None

    def next(self) -> dict:
        m, st = self.m, self.st
        kw, _, y, y_lo = m._res_layer_args(st.ws, "te", "text_encoder", st.pk, st.rs1, self.i, len(m.text_encoder.layers), self.x_f, self.x_p,
                                           self.x_lo, st.gap1.data_ptr(), m.split, False)
        self.i, self.x_f, self.x_p, self.x_lo = self.i + 1, None, y, y_lo
        return kw

    def ride(self, i: int) -> Optional[dict]:
        """`rider` of _res_stack: the remaining text layers share the launches of mel-encoder layers `ride_from` on"""
        return self.next() if i >= self.ride_from else None


class EfficientTTSCNN(torch.nn.Module):
    """EFTS-CNN acoustic model (drop-in for nntts.models.EfficientTTSCNN).

    Extra keyword (not in the reference): ``precision`` selects the MFMA operand mode of the
    Conv1d/Linear stacks: "bf16x3" (split-bf16, fp32-class accuracy; default), "bf16", or "fp32"
    (exact fp32 operands on the fp32-input MFMA, efts_gemm on format-3 planes: the reference-parity
    mode, eval paths only -- training refuses it).  The alignment block (QK^T, expand) runs in bf16x3
    in the bf16 / bf16x3 modes and in fp32 in the fp32 mode.  An fp32 model runs the generic fallback
    of every fused launch that has no fp32 form (FP32_GENERIC_OPTIONS are off, and setting one raises).
    """

    def __init__(self, num_symbols: int, odim: int = 80, symbol_embedding_dim: int = 512, n_channels: int = 512,
                 n_text_encoder_layer: int = 5, n_mel_encoder_layer: int = 3, n_decoder_layer: int = 6,
                 n_duration_layer: int = 2, k_size: int = 5, nonlinear_activation="LeakyReLU",
                 nonlinear_activation_params={"negative_slope": 0.1}, use_weight_norm=True, dropout_rate=0.1,
                 use_masking: bool = False, use_weighted_masking: bool = False, duration_offset=1.0, sigma=0.01,
                 sigma_e=0.5, delta_e_method_1=True, share_text_encoder_key_value=False, use_mel_query_fc=False,
                 precision: str = "bf16x3"):
        super().__init__()
        if precision not in PRECISIONS:
            raise ValueError(f"precision must be one of {list(PRECISIONS)}")
        # LeakyReLU (every reference config) and ReLU (= slope 0) live in the epilogues of the contraction kernels; the other pointwise
        # torch.nn activations run as a separate elementwise launch behind the contraction (csrc/efts_act.hip)
        act_general = None
        if nonlinear_activation == "ReLU" and set(nonlinear_activation_params) - {"inplace"}:
            # the reference builds torch.nn.ReLU(**params) (efts_modules.py:32-35): anything but `inplace` is a TypeError there
            raise TypeError(f"ReLU.__init__() got an unexpected keyword argument {sorted(set(nonlinear_activation_params) - {'inplace'})[0]!r}")
        if nonlinear_activation not in ("LeakyReLU", "ReLU") or set(nonlinear_activation_params) - {"negative_slope", "inplace"}:
            act_general = L.actfn(nonlinear_activation, dict(nonlinear_activation_params))
            if act_general is None:
                raise NotImplementedError(f"nonlinear_activation={nonlinear_activation!r}({nonlinear_activation_params}): the library has forms of "
                                          f"{sorted(L.ACTFN)} with their scalar parameters (learnable or non-pointwise modules have none)")
        if symbol_embedding_dim != n_channels:
            raise ValueError("symbol_embedding_dim must equal n_channels (the reference adds them residually)")
        if k_size % 2 == 0 or not 1 <= k_size <= 11:
            raise NotImplementedError("k_size must be odd and <= 11 (efts_gemm's tap counts; the guard rows in front of a row space hold "
                                      "a padding of up to 5).  5, the value of every reference config, and 3 run the mel-length stacks on "
                                      "efts_resconv5; 1, 7, 9 and 11 on efts_gemm")
        if use_weighted_masking:
            raise NotImplementedError("FastSpeechLoss(use_weighted_masking=True) is not implemented (no shipped config selects it)")
        if n_channels % 256 or odim > 128:
            raise NotImplementedError("n_channels must be a multiple of 256 and odim <= 128")
        self.precision = precision
        self.split = PRECISIONS[precision]
        self.align_split = L.SPLIT_FP32 if self.split == L.SPLIT_FP32 else L.SPLIT_BF16X3   # operand format of q, k, alpha'^T, V^T
        self.odim, self.n_channels, self.num_symbols = odim, n_channels, num_symbols
        self.duration_offset, self.sigma, self.sigma_e = duration_offset, sigma, sigma_e
        self.delta_e_method_1 = delta_e_method_1
        self.share_text_encoder_key_value = share_text_encoder_key_value
        self.use_masking = bool(use_masking)        # False (the reference ctor default): the two losses are means over the padded tensors
        self.k_size = int(k_size)
        self.row_gap = max(L.GAP, (self.k_size - 1) // 2)           # zero rows between the items of a row space (include/efts_abi.h "Row space")
        # LeakyReLU's own default slope is 0.01 (torch.nn.LeakyReLU); ReLU = slope 0 through the same epilogue
        self.slope = float(nonlinear_activation_params.get("negative_slope", 0.01)) if nonlinear_activation == "LeakyReLU" else 0.0
        self.act_general = act_general                                # (EFTS_ACTFN id, p0, p1) or None = the fused (Leaky)ReLU
        self.dropout_rate = dropout_rate
        a, ap = nonlinear_activation, nonlinear_activation_params
        # construction order == reference (efficient_tts.py:57-112) so a given torch seed
        # yields the reference's default initialisation
        self.text_embedding_table = torch.nn.Embedding(num_symbols, symbol_embedding_dim)
        self.text_encoder = _ResConvBlock(n_text_encoder_layer, n_channels, k_size, a, ap, dropout_rate, use_weight_norm)
        self.text_encoder_key = torch.nn.Linear(n_channels, n_channels)
        if not share_text_encoder_key_value:        # (:72-75) shared: the value IS the key projection
            self.text_encoder_value = torch.nn.Linear(n_channels, n_channels)
        self.mel_prenet = torch.nn.Sequential(torch.nn.Linear(odim, n_channels), getattr(torch.nn, a)(**ap),
                                              torch.nn.Dropout(dropout_rate))
        self.mel_encoder = _ResConvBlock(n_mel_encoder_layer, n_channels, k_size, a, ap, dropout_rate, use_weight_norm)
        self.mel_query_fc = torch.nn.Linear(n_channels, n_channels) if use_mel_query_fc else None      # (:90-95)
        self.decoder = _ResConvBlock(n_decoder_layer, n_channels, k_size, a, ap, dropout_rate, use_weight_norm)
        self.mel_output_layer = torch.nn.Linear(n_channels, odim)
        self.duration_predictor = _DurationPredictor(n_channels, n_duration_layer, n_channels, offset=duration_offset)
        self.opt = LaunchOptions()          # launch-affecting options (A/B and test hooks): also plain attributes of the model, see below
        if self.split == L.SPLIT_FP32:
            for name in FP32_GENERIC_OPTIONS:
                setattr(self.opt, name, False)
        self._free_running = False          # set while inference() / inference_batch() enqueue their launches
        self.graphs = True                  # plain eval calls replay a per-shape hipGraph (False: every kernel launched eagerly)
        self._graph_cache = GraphCache()
        self.graph_policy = "auto"          # teacher-forced forward: "auto" = a shape replays a graph only where launch latency is not
                                            # hidden by the device time anyway (graphs.GraphCache.run, adaptive); "always" = every shape
        self._len1 = {}
        self._infer_cache = GraphCache(capacity=64)      # free-running inference: two phases per (bucketed) shape
        self.dropout_seed = 0x5EED          # base seed of the train-mode dropout masks (mixed with the data-parallel rank and the step counter)
        self.dropout_calls = 0              # training steps taken so far: the position in the mask sequence (the trainer restores it from the step count on --resume)
        self._probed_at, self._probe_calls = 0, 0      # gradient-free train()-mode passes since `dropout_calls` was _probed_at (probe_dropout)
        self.planes = WeightPlanes()        # the packed operand planes of the Conv1d / Linear weights
        self._ws: Dict[Tuple, _Workspace] = {}
        self._ws_infer: Dict[Tuple, _Workspace] = {}
        self._ws_train: Dict[Tuple, _Workspace] = {}

    # ------------------------------------------------------------------ weight norm (efficient_tts.py:400-418)
    def remove_weight_norm(self):
        for m in self.modules():
            if isinstance(m, torch.nn.Conv1d) and hasattr(m, "weight_g"):
                torch.nn.utils.remove_weight_norm(m)
                logging.debug(f"Weight norm is removed from {m}.")
        self.planes.invalidate()

    def apply_weight_norm(self):
        for m in self.modules():
            if isinstance(m, torch.nn.Conv1d) and not hasattr(m, "weight_g"):
                torch.nn.utils.weight_norm(m)
        self.planes.invalidate()

    # ------------------------------------------------------------------ packed weights (weights.py)
    def _te0_table(self, drop: DropoutPlan = NONE) -> Optional[torch.Tensor]:
        """tap table of text-encoder layer 0 (WeightPlanes.te0_table) where the look-up form applies, else None"""
        if not self.embed_conv or len(self.text_encoder.layers) == 0 or self.n_channels % 32 or drop.conv_active or self.k_size > 5 or self.act_general:
            return None                      # (a Dropout mask sits between layer 0's activation and its residual add: no look-up form)
        return self.planes.te0_table(self)

    def _embed_te0(self, ws, pk, text, rs1: Rows, lens_i32: Optional[torch.Tensor], tab: torch.Tensor):
        """embedding + text-encoder layer 0 in one gather launch -> (fp32 stream, operand plane) of layer 0's output"""
        C = self.n_channels
        x_f, x_p = ws.f32("te_f0", rs1, C), ws.plane("te_p0", rs1, C, self.split)
        O.embed_conv(text, lens_i32, self.text_embedding_table.weight.detach(), tab, self.text_encoder.layers[0].conv[0].bias, self.slope,
                     x_f, x_p, rs1)
        return x_f, x_p

    # ------------------------------------------------------------------ train-mode Dropout (counter-based masks: dropout.py)
    def _dropout_plan(self, calls: int, step_word_ptr: Optional[int] = None) -> DropoutPlan:
        """the masks of step `calls`: in train() mode the duration predictor's Dropout(0.1) always (duration_predictor.py:61), the convs' with dropout_rate"""
        conv_p = float(self.dropout_rate) if self.training and self.dropout_rate >= 1e-5 else 0.0
        dur_p = float(self.duration_predictor.conv[0][3].p) if self.training else 0.0
        return DropoutPlan(conv_p, dur_p, rank_base(self.dropout_seed, dist_rank()), calls, step_word_ptr)

    def step_dropout(self, step_word_ptr: Optional[int] = None) -> DropoutPlan:
        """a training step: moves the mask sequence on and returns the step's masks (step_word_ptr: see DropoutPlan)"""
        self.dropout_calls = int(self.dropout_calls) + 1
        return self._dropout_plan(self.dropout_calls, step_word_ptr)

    def probe_dropout(self) -> DropoutPlan:
        """A gradient-free pass in train() mode (a probe, a validation pass that forgot eval()) does NOT advance `dropout_calls`: that counter
        sequences the masks of the optimisation steps (GraphedStep's step words, the trainer's --resume), and a resumed run must reproduce the
        uninterrupted one.  Probes draw the step that comes next, then the ones behind it; their counter restarts when a real step has moved on"""
        if self._probed_at != int(self.dropout_calls):
            self._probed_at, self._probe_calls = int(self.dropout_calls), 0
        self._probe_calls += 1
        return self._dropout_plan(self._probed_at + self._probe_calls)

    def _side_stream(self, device) -> "torch.cuda.Stream":
        if not self.side_stream:
            return torch.cuda.current_stream(device)
        st = getattr(self, "_side", None)
        if st is None or st.device != device:
            st = torch.cuda.Stream(device=device)
            object.__setattr__(self, "_side", st)
        return st

    def _aux_stream(self, device) -> "torch.cuda.Stream":
        """a third stream (the training pass: the decoder's grouped weight gradients beside the alignment block's backward)"""
        if not self.side_stream:
            return torch.cuda.current_stream(device)
        st = getattr(self, "_aux", None)
        if st is None or st.device != device:
            st = torch.cuda.Stream(device=device)
            object.__setattr__(self, "_aux", st)
        return st

    def _workspace(self, key, device, pin=()) -> _Workspace:
        """The buffers of one shape.  Bounded LRU pools (each entry holds full activations): 4 teacher-forced / training
        shapes, 64 free-running ones (one or a few utterances, a few MB each).  `pin`: workspaces of the call in progress,
        never evicted -- their buffers are about to be read (the value projection of phase 1) or captured."""
        if key[0] in ("infb", "infb2", "inf", "inf2"):
            pool, cap = self._ws_infer, 64
        elif key[0] == "train":
            # training shapes have a pool of their own: an evaluation pass over more than four shapes must not evict the workspace a
            # captured training step (step_graph.GraphedStep) points into -- that forces a recapture and keeps two multi-GB
            # workspaces alive at once
            pool, cap = self._ws_train, 4
        else:
            pool, cap = self._ws, 4
        ws = pool.pop(key, None)
        if ws is None:
            for old in list(pool):
                if len(pool) < cap:
                    break
                if not any(pool[old] is q for q in pin):
                    del pool[old]
            ws = _Workspace(device)
        pool[key] = ws                                   # most recently used last
        return ws

    # ------------------------------------------------------------------ building blocks

    def _til(self, rows: int):
        """efts_gemm tiling for a 512-column launch over `rows` rows: the small-M kernel (64 x 32 tiles, K split across the waves:
        ~4x shorter dependent chain per layer) for one-utterance row spaces of the free-running path, else the library's rules"""
        if self._free_running and self.small_m and rows <= self.SMALL_M_ROWS and self.n_channels % 32 == 0 and self.k_size <= 5:
            return L.TILING_SMALLM
        return None

    def _on_resconv(self, rs: Rows, drop: DropoutPlan = NONE) -> bool:
        if drop.conv_active:                 # conv Dropout in this pass: efts_gemm's epilogue carries the masks
            return False
        return self.resconv and rs.rows >= self.RESCONV_MIN_ROWS and self.n_channels % 256 == 0 and self.k_size in (3, 5) and self.act_general is None

    def _stream_in(self, ws, tag, rs: Rows, drop: DropoutPlan = NONE):
        """Buffers the producer of a residual stack's input writes: (fp32 stream or None, operand plane, lo plane or None).
        A stack on efts_resconv5 reads its residual from the planes, so no fp32 copy is written at all."""
        C = self.n_channels
        pl = ws.plane(f"{tag}_p", rs, C, self.split)
        if self._on_resconv(rs, drop):
            return None, pl, (ws.plane(f"{tag}_l", rs, C, 1) if self.split == 1 else None)
        return ws.f32(f"{tag}_f", rs, C), pl, None

    def _res_layer_args(self, ws, tag, blk, pk, rs: Rows, i: int, n: int, x_f32, x_pl: Plane, x_lo, gap_ptr, last_split: int, last_f32: bool):
        """keyword set of efts_resconv5 for layer i of a stack on hi / lo planes, and the buffers it writes (`x_f32`: the fp32
        stream to take the residual from instead of the planes, or None)"""
        C = self.n_channels
        last = i == n - 1
        o_split = last_split if last else self.split
        y = ws.plane(f"{tag}_p{i & 1}", rs, C, o_split)
        y_lo = ws.plane(f"{tag}_l{i & 1}", rs, C, 1) if (o_split == 1 and not last) else None
        o_f32 = ws.f32(f"{tag}_f{i & 1}", rs, C) if (last and last_f32) else None
        kw = dict(x=x_pl, x_lo=x_lo, x_f32_ptr=None if x_f32 is None else x_f32.ptr, ldr=C, w=pk[f"{blk}.{i}"], taps=self.k_size,
                  m=rs.rows, n=C, bias=getattr(self, blk).layers[i].conv[0].bias, slope=self.slope,
                  rowmask_ptr=gap_ptr, y_f32_ptr=None if o_f32 is None else o_f32.ptr, ldo=C, y=y, y_lo=y_lo)
        return kw, o_f32, y, y_lo

    def _res_stack(self, ws, tag, blk, pk, rs: Rows, x_f32: Optional[F32Rows], x_pl: Plane, gap_ptr, last_split: int,
                   last_f32: bool, x_lo: Optional[Plane] = None, rider=None, after=None, start: int = 0, drop: DropoutPlan = NONE):
        """n x ( x + LeakyReLU(conv1d_k5(x)) ) on the row space (efts_modules.py:48-51,77-79).
        `rider(i)`: optional, returns the efts_resconv5 keyword set of an independent layer of the same geometry that shares
        layer i's persistent launch (or None); `after(i)`: optional, called when layer i's launch has been enqueued; `start`: first
        layer to run (x is then the output of layer start - 1)."""
        n = len(getattr(self, blk).layers)
        C = self.n_channels
        if self._on_resconv(rs, drop):
            # The stream between the layers is a pair of bf16 planes (hi = the next layer's MFMA operand, lo = the
            # remainder; split 2 planes carry both): 4 B read + 4 B written per element and layer instead of 4 + 6..8 B.
            o_f32 = None
            for i in range(start, n):
                kw, o_f32, y, y_lo = self._res_layer_args(ws, tag, blk, pk, rs, i, n, x_f32 if i == start else None, x_pl, x_lo, gap_ptr, last_split, last_f32)
                extra = rider(i) if rider is not None else None
                if extra is not None:
                    O.resconv5_multi([kw, extra])
                else:
                    O.resconv5(**kw)
                if after is not None:
                    after(i)
                x_pl, x_lo = y, y_lo
            return o_f32, x_pl
        assert rider is None and after is None
        for i in range(start, n):
            last = i == n - 1
            w = pk[f"{blk}.{i}"]
            o_split = last_split if last else self.split
            o_f32 = ws.f32(f"{tag}_f{i & 1}", rs, C) if (not last or last_f32) else None
            o_pl = ws.plane(f"{tag}_p{i & 1}", rs, C, o_split)
            dp_, dseed = drop.conv(LAUNCH.get(tag, LAUNCH["other"]) + i)      # efts_modules.py:38-47: Dropout behind the activation, in front of the residual add
            if self.act_general is not None:                 # any other torch.nn activation: pre-activation in fp32, then one elementwise launch
                z = ws.f32(f"{tag}_z", rs, C)
                O.gemm(a=x_pl, b_ptr=w.ptr, ldb=w.ld, b_tap_stride=w.tap_stride, taps=self.k_size, m=rs.rows, n=C,
                       bias=getattr(self, blk).layers[i].conv[0].bias, out_f32_ptr=z.ptr, ldo=C, tiling=self._til(rs.rows))
                o_f32 = ws.f32(f"{tag}_f{i & 1}", rs, C)
                O.act_apply(self.act_general, z.ptr, x_f32.ptr, gap_ptr, o_f32, o_pl, rs.rows, C, dp_, dseed)
                x_f32, x_pl = o_f32, o_pl
                continue
            O.gemm(a=x_pl, b_ptr=w.ptr, ldb=w.ld, b_tap_stride=w.tap_stride, taps=self.k_size, m=rs.rows, n=C,
                   act=L.ACT_LEAKY, slope=self.slope, bias=getattr(self, blk).layers[i].conv[0].bias,
                   resid_ptr=x_f32.ptr, ldr=C, rowmask_ptr=gap_ptr,
                   out_f32_ptr=None if o_f32 is None else o_f32.ptr, ldo=C, out_plane=o_pl, tiling=self._til(rs.rows),
                   drop_p=dp_, drop_seed=dseed)
            x_f32, x_pl = o_f32, o_pl
        return x_f32, x_pl

    def _embed_text(self, ws, pk, text, rs1: Rows, lens: Optional[torch.Tensor], mask: Optional[torch.Tensor], drop: DropoutPlan = NONE) -> _Embedded:
        """The embedding (efficient_tts.py:144 / :246), or the embedding + text-encoder layer 0 as table look-ups where that form applies.
        lens (int32 [B]) / mask (the row mask `len1`): zero beyond each item's length (the ragged free-running path); both None: padded
        ids are real symbols (the teacher-forced forward)"""
        C = self.n_channels
        tab = self._te0_table(drop)
        if tab is not None:
            return _Embedded(*self._embed_te0(ws, pk, text, rs1, lens, tab), 1)
        table = self.text_embedding_table.weight.detach()
        if mask is None:
            x_f, x_p = ws.f32("emb_f", rs1, C), ws.plane("emb_p", rs1, C, self.split)
            O.embed(text, table, x_f, x_p, rs1)
        else:
            e_f = ws.f32("emb_raw", rs1, C)
            O.embed(text, table, e_f, None, rs1)
            x_f, x_p = ws.f32("emb_f", rs1, C), ws.plane("emb_p", rs1, C, self.split)
            O.mask_rows(e_f.ptr, mask.data_ptr(), x_f, x_p, rs1.rows, C)
        return _Embedded(x_f, x_p, 0)

    def _text_stack(self, ws, pk, rs1: Rows, emb: _Embedded, mask_ptr, drop: DropoutPlan = NONE) -> Plane:
        """the text-encoder layers behind `emb` (efficient_tts.py:148 / :250) -> the operand plane of the last one"""
        if emb.start >= len(self.text_encoder.layers):
            return emb.x_p
        return self._res_stack(ws, "te", "text_encoder", pk, rs1, emb.x_f, emb.x_p, mask_ptr, self.split, False, start=emb.start, drop=drop)[1]

    def _text_side(self, ws, pk, text, rs1: Rows, gap1, len1, vt: Optional[Plane] = None) -> _TextSide:
        """embed -> text encoder -> key (split-2 plane, masked), value (fp32 + plane, masked)
        (efficient_tts.py:144-157 / :246-255) on one stream; `vt`: also pack V^T for the alpha'.V launch here."""
        h_p = self._text_stack(ws, pk, rs1, self._embed_text(ws, pk, text, rs1, None, None), gap1.data_ptr())
        key_p = self._key_proj(ws, pk, rs1, h_p, gap1, len1)
        return _TextSide(key_p, *self._value_proj(ws, pk, rs1, h_p, gap1, len1, vt))

    def _key_proj(self, ws, pk, rs1: Rows, h_p: Plane, gap1, len1) -> Plane:
        """text_encoder_key, zero at padded text (efficient_tts.py:149, :155-156): split-2 operand plane of q.k^T"""
        C = self.n_channels
        key_p = ws.plane("key_p", rs1, C, self.align_split)
        wk = pk["key"]
        O.gemm(a=h_p, b_ptr=wk.ptr, ldb=wk.ld, m=rs1.rows, n=C, bias=self.text_encoder_key.bias,
               rowmask_ptr=(gap1 if len1 is None else len1).data_ptr(), out_plane=key_p, tiling=self._til(rs1.rows))
        return key_p

    def _value_proj(self, ws, pk, rs1: Rows, h_p: Plane, gap1, len1, vt: Optional[Plane] = None):
        """text_encoder_value (the key projection again when shared, :150-153), zero at padded text (:157): fp32 + operand plane"""
        C = self.n_channels
        val_f = ws.f32("val_f", rs1, C)
        val_p = ws.plane("val_p", rs1, C, self.split)
        shared = self.share_text_encoder_key_value
        wv = pk["key"] if shared else pk["value"]
        vbias = self.text_encoder_key.bias if shared else self.text_encoder_value.bias
        O.gemm(a=h_p, b_ptr=wv.ptr, ldb=wv.ld, m=rs1.rows, n=C, bias=vbias,
               rowmask_ptr=(gap1 if len1 is None else len1).data_ptr(), out_f32_ptr=val_f.ptr, ldo=C, out_plane=val_p, tiling=self._til(rs1.rows))
        if vt is not None:
            O.pack_vt(val_f, vt, rs1.B, rs1.T, rs1.Tp, C)
        return val_f, val_p

    def _duration(self, ws, pk, rs1: Rows, val_p: Plane, gap1, out_mask_ptr, mode: int, drop: DropoutPlan = NONE) -> torch.Tensor:
        """DurationPredictor._forward (duration_predictor.py:66-88); its Dropout(0.1) behind each LayerNorm (:61) is applied with the
        masks of `drop` (a train()-mode pass), else identity."""
        C = self.n_channels
        dp = self.duration_predictor
        h_f = ws.f32("dur_f", rs1, C)
        x_p = val_p
        for i, seq in enumerate(dp.conv):
            w = pk[f"dur.{i}"]
            O.gemm(a=x_p, b_ptr=w.ptr, ldb=w.ld, b_tap_stride=w.tap_stride, taps=3, m=rs1.rows, n=C, act=L.ACT_RELU,
                   bias=seq[0].bias, out_f32_ptr=h_f.ptr, ldo=C, tiling=self._til(rs1.rows))
            x_p = self._duration_norm(ws, rs1, i, gap1, out_mask_ptr, mode, drop)
        return ws.tensor("dur_out", (rs1.rows,))

    def _duration_norm(self, ws, rs1: Rows, i: int, gap1, out_mask_ptr, mode: int, drop: DropoutPlan = NONE) -> Optional[Plane]:
        """LayerNorm behind conv i (duration_predictor.py:58-61): -> the next conv's operand plane, or (last layer) + Linear(C, 1) ->
        the predicted log-durations in ws "dur_out" """
        C = self.n_channels
        dp = self.duration_predictor
        ln = dp.conv[i][2]
        h_f = ws.f32("dur_f", rs1, C)
        if i + 1 < len(dp.conv):
            x_p = ws.plane(f"dur_p{i}", rs1, C, self.split)
            O.layernorm_rows(h_f.ptr, ln.weight.detach(), ln.bias.detach(), ln.eps, gap1.data_ptr(), None, x_p, rs1.rows, C, *drop.dur(i))
            return x_p
        O.layernorm_dot(h_f.ptr, ln.weight.detach(), ln.bias.detach(), ln.eps, dp.linear.weight.detach(), dp.linear.bias.detach(),
                        out_mask_ptr, mode, float(dp.offset), ws.tensor("dur_out", (rs1.rows,)), rs1.rows, C, *drop.dur(i))
        return None

    def _fused_expand(self, T1: int) -> bool:
        return self.fuse_expand and T1 <= 256 and self.n_channels % 128 == 0

    def _expand_decode(self, ws, pk, B, T1, rs1: Rows, rs2: Rows, val_f: F32Rows, e, tl, ml, ralpha, len2_ptr, gap2,
                       vt: Optional[Plane] = None, rider=None, after=None, loss_target: Optional[torch.Tensor] = None, drop: DropoutPlan = NONE):
        """Gaussian re-alignment from e, bmm(V^T, alpha') -> decoder -> mel head (efficient_tts.py:184-200 / :270-284).
        `ralpha` [B, T1, T2] receives alpha' (the API tensor); tl / ml: int32 lengths or None (no masks, :270-274);
        `vt`: V^T already packed (unfused path only); `loss_target`: the frames of the loss's mel term, which the head's epilogue takes
        where its launch fills the chip.  -> _Head: the mel and the squared-error partials that epilogue left (or None, 0)."""
        C = self.n_channels
        h_f, h_p, h_l = self._stream_in(ws, "exp", rs2, drop)
        if self._fused_expand(T1):
            # alpha' is the MFMA A operand, produced in registers; V is read as fp32: no alpha'^T plane, no V^T planes
            O.expand(e=e, tl=tl, ml=ml, sigma=float(self.sigma), v=val_f, rs1=rs1, rs2=rs2, alpha_out=ralpha, y_f32=h_f, y=h_p, y_lo=h_l)
        else:
            ra_plane = ws.plane("ra_p", rs2, T1, self.align_split)
            O.reconst_alpha(e, tl, ml, float(self.sigma), ralpha, ra_plane, B, T1, rs2.T, rs2.Tp)
            if vt is None:
                vt = ws.raw_plane("vt", B * C, T1, self.align_split)
                O.pack_vt(val_f, vt, B, T1, rs1.Tp, C)
            O.gemm(a=ra_plane, b_ptr=vt.ptr, ldb=vt.ld, m=rs2.T, n=C, batch=B, a_batch_stride=rs2.Tp * ra_plane.ld,
                   b_batch_stride=C * vt.ld, rowmask_ptr=len2_ptr, rowmask_batch_stride=rs2.Tp,
                   out_f32_ptr=None if h_f is None else h_f.ptr, ldo=C, out_batch_stride=rs2.Tp * C, out_plane=h_p,
                   outb_batch_stride=rs2.Tp * h_p.ld, out_plane_lo=h_l)
        _, d_p = self._res_stack(ws, "dec", "decoder", pk, rs2, h_f, h_p, gap2.data_ptr(), self.split, False, x_lo=h_l, rider=rider, after=after, drop=drop)
        # mel head (:198-200), written straight into the [B, T2, odim] tensor the caller gets (one item per batch entry of the
        # launch: no row-space copy of mel_pred, no clone)
        mel = torch.empty(B, rs2.T, self.odim, dtype=torch.float32, device=h_p.buf.device)
        wh = pk["head"]
        loss_kw, part, n_part = {}, None, 0
        if loss_target is not None and self.fuse_mel_loss and self.use_masking and len2_ptr is not None and self.odim % 4 == 0 and self.odim <= 128:
            # the mel term of the loss (:220, fastspeech_loss.py:54-67) in the head's epilogue: the tile is in LDS, the target frames arrive
            # where a residual would, the row mask IS the loss mask -- one launch less at the end of every forward.  Only where AUTO picks the
            # generic tiling anyway (one workgroup per CU or more): a short launch keeps its 64-column tiles and the separate loss launch
            mt = (rs2.T + 127) // 128
            if B * mt >= (self.fuse_mel_loss_min_wgs or torch.cuda.get_device_properties(mel.device).multi_processor_count):
                part, n_part = ws.tensor("sqerr_part", (B * mt * 4,)), B * mt * 4
                loss_kw = dict(sqerr_target=loss_target, sqerr_part=part)
        O.gemm(a=d_p, b_ptr=wh.ptr, ldb=wh.ld, m=rs2.T, n=self.odim, batch=B, a_batch_stride=rs2.Tp * d_p.ld, bias=self.mel_output_layer.bias,
               rowmask_ptr=len2_ptr if len2_ptr is not None else gap2.data_ptr(), rowmask_batch_stride=rs2.Tp,
               out_f32_ptr=mel.data_ptr(), ldo=self.odim, out_batch_stride=rs2.T * self.odim, **loss_kw)
        return _Head(mel, part, n_part)

    def _require(self, t: torch.Tensor):
        if not t.is_cuda:
            raise L.EftsError("EfficientTTSCNN runs on an MI355X only: inputs/parameters must be on a ROCm device "
                              "(there is no CPU fallback)")
        L.require_device()

    # ------------------------------------------------------------------ forward (efficient_tts.py:120-228)
    def forward(self, text: torch.Tensor, text_lengths: torch.Tensor, speech: torch.Tensor,
                speech_lengths: torch.Tensor):
        """Teacher-forced forward.  Returns (loss, stats, imv[B,T2], reconst_alpha[B,T1,T2],
        mel_pred[B,T2,odim], speech) exactly like the reference (:228)."""
        training_path = torch.is_grad_enabled() and (self.text_embedding_table.weight.requires_grad or any(p.requires_grad for p in self.parameters()))
        self._require(text)
        if training_path:
            require_trainable(self, "EfficientTTSCNN.forward with gradients")
            from .autograd import training_forward
            return training_forward(self, text, text_lengths, speech, speech_lengths)
        if self.training:
            # train() mode without gradients (a validation pass that forgot eval(), a probe): the reference applies its Dropouts here --
            # the duration predictor's 0.1 always (duration_predictor.py:61), ResConv1d's and the prenet's when dropout_rate > 0
            # (efts_modules.py:38-47, efficient_tts.py:76-80).  Same counter-based masks as the fused training pass would draw for the
            # next step (`probe_dropout`: `dropout_calls` itself is left alone); the seeds are by-value launch arguments, so no graph
            return self._forward_impl(text, text_lengths, speech, speech_lengths)[0]
        if not self.graphs or torch.cuda.is_current_stream_capturing():
            return self._forward_impl(text, text_lengths, speech, speech_lengths)[0]
        # per-shape hipGraph: the launches of this shape are replayed as one graph (efficient_tts_amd/graphs.py)
        self.planes.get(self)                                 # (re)packing stays outside the graph
        self._te0_table()                                     # ... and so does the tap table of text-encoder layer 0
        dev = text.device
        key = ("fwd", tuple(text.shape), tuple(speech.shape), text.dtype, speech.dtype, text_lengths.dtype, speech_lengths.dtype)
        ws = self._workspace(("fwd", text.shape[0], text.shape[1], speech.shape[1]), dev)
        # the graph is valid while the buffers its launches point at live: this workspace, the packed planes, the parameters
        tag = (ws.serial, self.planes.tag(), self.opt.tag())

        def body(t, tl, sp, sl):
            (_, stats, imv, ralpha, mel_pred, _), _ = self._forward_impl(t, tl, sp, sl)
            return stats._t, imv, ralpha, mel_pred

        out3, imv, ralpha, mel_pred = self._graph_cache.run(key, tag, (text, text_lengths.to(dev), speech, speech_lengths.to(dev)), body, keepalive=ws,
                                                            adaptive=self.graph_policy == "auto")
        return out3[0], LazyStats(out3), imv, ralpha, mel_pred, speech

    def _forward_impl(self, text, text_lengths, speech, speech_lengths, keep: bool = False):
        with O.stream_scope():
            return self._forward_body(text, text_lengths, speech, speech_lengths, keep, self.probe_dropout() if self.training else NONE)

    # ------------------------------------------------------------------ the schedule of the forward: every stage call, fork, hand-over and join
    def _forward_body(self, text, text_lengths, speech, speech_lengths, keep: bool = False, drop: DropoutPlan = NONE):
        """The whole teacher-forced forward.  Two HIP streams: the text side (masks, embed, 5 convs, K/V) and the duration predictor do
        not depend on the mel side (prenet, 3 convs) and run on `side` beside the mel-length kernels on `main`."""
        st = self._begin_forward(text, text_lengths, speech, speech_lengths, drop)      # masks on main
        fr, al = self._to_alignment(st, keep, full=True)
        ralpha = torch.empty(st.B, st.T1, st.T2, dtype=torch.float32, device=st.text.device)
        st.main.wait_event(fr.v_ready)                                          # V from the side stream
        head = self._expand_decode(st.ws, st.pk, st.B, st.T1, st.rs1, st.rs2, fr.val_f, al.e, st.tl, st.ml, ralpha, st.len2.data_ptr(), st.gap2,
                                   vt=st.vt, loss_target=st.speech, drop=st.drop)       # :184-200
        st.main.wait_stream(st.side)                                            # duration predictor done
        out3 = self._losses(st, head, fr.dur, al.lde)                           # :220-227
        # (for inspection only -- tests look whether the head's epilogue took the loss's mel term; nothing reads it back)
        object.__setattr__(self, "_sqerr_parts", None if head.sqerr_part is None else (head.sqerr_part, head.n_part))
        ret = (out3[0], LazyStats(out3), al.imv, ralpha, head.mel, st.speech)
        extra = dict(e=al.e, log_delta_e=al.lde, dur_pred=fr.dur.view(st.B, st.rs1.Tp)[:, :st.T1], ws=st.ws) if keep else None
        return ret, extra

    def _align_body(self, text, text_lengths, speech, speech_lengths) -> Tuple[_Pass, _Aligned]:
        """The forward through the IMV block and nothing behind it (align()): no decoder, mel head or losses, and none of the launches
        only they read.  al.e is the workspace's buffer."""
        st = self._begin_forward(text, text_lengths, speech, speech_lengths)
        _, al = self._to_alignment(st, False, full=False)
        st.main.wait_stream(st.side)
        return st, al

    def _to_alignment(self, st: _Pass, keep: bool, full: bool) -> Tuple[_Front, _Aligned]:
        """fork, both encoders on their streams, K behind the mel encoder, then the alignment block on main.  full False: without what
        only the decoder and the losses read (_front_merged, _front_split)"""
        st.side.wait_stream(st.main)
        merged = self._on_resconv(st.rs2, st.drop) and len(self.text_encoder.layers) >= 1 and len(self.mel_encoder.layers) >= 1
        fr = self._front_merged(st, full) if merged else self._front_split(st, full)
        sidx, alpha = self._soft_index(st, fr.q_p, fr.key_p, keep)
        return fr, self._imv(st, sidx, alpha)

    def _front_merged(self, st: _Pass, full: bool) -> _Front:
        """Long row spaces.  The last min(nt, nm) text-encoder layers ride in the persistent launches of the mel-encoder layers (one
        grouped efts_resconv5_multi launch per pair: the text rows are scheduled behind the mel rows at the long launch's efficiency).
        A persistent launch owns every CU's LDS, so a text-length launch of its own beside it would get the 4 spare CUs: only the
        first nt - nm text layers run by themselves (efts_resconv5 on the short row space), beside the HBM-bound prenet on the second
        stream.  full False skips the value projection and the duration predictor."""
        main, side = st.main, st.side
        nt, nm = len(self.text_encoder.layers), len(self.mel_encoder.layers)
        first = 0 if self._te0_table(st.drop) is None else 1                   # (layer 0 may be table look-ups: it never rides)
        nr = min(nt - first, nm)
        ns = nt - nr                                                           # text layers that run by themselves first
        # The first text layers and the prenet share the chip by halves: both kinds of workgroup take a whole CU (LDS), the
        # prenet is bound by HBM -- which half the CUs saturate -- and a text-length layer by streaming its weights, so the
        # prenet's grid is capped at half the CUs and the text layers are scheduled onto the other half.
        cus = torch.cuda.get_device_properties(st.text.device).multi_processor_count
        share = ns > first and cus >= 64
        with O.on_stream(side):
            pre = self._prenet(st, cus // 2 if share else 0)                   # (r6: 128 / 144 / 160 / 176 CUs for the prenet measured: no difference)
            pre_ready = O.hand_over(side)
        te_plan = O.resconv5_plan_buf(st.rs1.rows, self.n_channels, cus // 2 - 2) if share else None      # (a host-side table: no launch)
        if not st.masks_done:
            O.row_masks(st.tl, st.rs1, st.gap1, st.len1)                       # :137 (behind the fork, on main: beside the prenet)
        cur = _TextCursor(self, st, self._embed_text(st.ws, st.pk, st.text, st.rs1, None, None, st.drop), ride_from=nm - nr)    # :144
        self._text_layers_alone(cur, ns, te_plan)                              # :148
        main.wait_event(pre_ready)
        q_p = self._mel_stack(st, pre, rider=cur.ride)
        te_done = O.hand_over(main)
        key_p = self._key_proj(st.ws, st.pk, st.rs1, cur.x_p, st.gap1, st.len1)       # :149, :155-156 (q.k^T is next on this stream)
        side.wait_event(te_done)
        val_f = dur = v_ready = None
        if full:
            # the value projection beside the key projection, then the duration predictor (needed by the loss only).  (Its k3
            # convolutions as riders of decoder launches: measured slower, 1.665 vs 1.633 ms, r3.)
            with O.on_stream(side):
                val_f, val_p = self._value_proj(st.ws, st.pk, st.rs1, cur.x_p, st.gap1, st.len1, st.vt)      # :150-157
                v_ready = O.hand_over(side)
                dur = self._duration(st.ws, st.pk, st.rs1, val_p, st.gap1, st.len1.data_ptr(), 0, st.drop)   # :219
        return _Front(q_p, key_p, val_f, dur, v_ready)

    def _front_split(self, st: _Pass, full: bool) -> _Front:
        """Short row spaces.  The text-side launches, on the second HIP stream, fill the tail rounds of the mel-length kernels; the
        q.k^T launch waits for the key projection, not for the value.  full False skips the duration predictor."""
        ws, pk, rs1, gap1, len1, side = st.ws, st.pk, st.rs1, st.gap1, st.len1, st.side
        with O.on_stream(side):
            if not st.masks_done:
                O.row_masks(st.tl, rs1, gap1, len1)                            # :137 (behind the fork, on side)
            h_p = self._text_stack(ws, pk, rs1, self._embed_text(ws, pk, st.text, rs1, None, None, st.drop), gap1.data_ptr(), st.drop)    # :144-148
            key_p = self._key_proj(ws, pk, rs1, h_p, gap1, len1)               # :149, :155-156
            k_ready = O.hand_over(side)
            val_f, val_p = self._value_proj(ws, pk, rs1, h_p, gap1, len1, st.vt)      # :150-157
            v_ready = O.hand_over(side)
            dur = self._duration(ws, pk, rs1, val_p, gap1, len1.data_ptr(), 0, st.drop) if full else None     # :219
        q_p = self._mel_stack(st, self._prenet(st))
        st.main.wait_event(k_ready)
        return _Front(q_p, key_p, val_f, dur, v_ready)

    # ------------------------------------------------------------------ the stages of the forward (launches on the current stream; no fork, no join)
    def _begin_forward(self, text, text_lengths, speech, speech_lengths, drop: DropoutPlan = NONE) -> _Pass:
        """workspace, row spaces, streams and the masks that go in front of the fork: both row spaces' in one launch, else (lengths of
        two dtypes) the mel mask only -- the prenet on the side stream reads gap2"""
        dev = text.device
        B, T1 = text.shape
        T2 = speech.shape[1]
        text = text.contiguous()
        speech = speech.contiguous().float()
        pk = self.planes.get(self)
        ws = self._workspace(("fwd", B, T1, T2), dev)
        rs1, rs2 = Rows(B, T1, self.row_gap), Rows(B, T2, self.row_gap)
        gap1, len1 = ws.tensor("gap1", (rs1.rows,)), ws.tensor("len1", (rs1.rows,))
        gap2, len2 = ws.tensor("gap2", (rs2.rows,)), ws.tensor("len2", (rs2.rows,))
        tl, ml, masks_done = lengths_and_masks(text_lengths, speech_lengths, dev, rs1, rs2, gap1, len1, gap2, len2)   # :137-139
        if not masks_done:
            O.row_masks(ml, rs2, gap2, len2)                                   # :139
        vt = None if self._fused_expand(T1) else ws.raw_plane("vt", B * self.n_channels, T1, self.align_split)
        return _Pass(ws=ws, pk=pk, text=text, speech=speech, B=B, T1=T1, T2=T2, rs1=rs1, rs2=rs2, gap1=gap1, len1=len1, gap2=gap2, len2=len2,
                     tl=tl, ml=ml, main=torch.cuda.current_stream(dev), side=self._side_stream(dev), vt=vt, masks_done=masks_done, drop=drop)

    def _prenet(self, st: _Pass, max_wgs: int = 0) -> _Prenet:
        """mel_prenet (:161) -> the mel encoder's input buffers.  max_wgs: cap of the fused launch's grid (0: none)"""
        ws, pk, rs2, speech, gap2, C = st.ws, st.pk, st.rs2, st.speech, st.gap2, self.n_channels
        pre_f, pre_p, pre_l = self._stream_in(ws, "pre", rs2, st.drop)
        wp = pk["prenet"]
        pre_dp, pre_seed = st.drop.conv(LAUNCH["prenet"])                      # mel_prenet's Dropout (:76-80)
        if self.act_general is not None:
            mel_in = ws.plane("mel_in", rs2, self.odim, self.split)
            O.pack_rows(speech, None, mel_in, rs2)
            z = ws.f32("pre_z", rs2, C)
            O.gemm(a=mel_in, b_ptr=wp.ptr, ldb=wp.ld, m=rs2.rows, n=C, bias=self.mel_prenet[0].bias, out_f32_ptr=z.ptr, ldo=C)
            O.act_apply(self.act_general, z.ptr, None, gap2.data_ptr(), pre_f, pre_p, rs2.rows, C, pre_dp, pre_seed)
        elif pre_dp == 0.0 and self.fuse_prenet and self.odim % 8 == 0 and self.odim <= 128 and C % 128 == 0:
            # straight from the caller's fp32 frames: no operand plane of the mel input, one launch (bit-identical on every frame)
            O.frame_linear(x=speech, w=wp, bias=self.mel_prenet[0].bias, act=L.ACT_LEAKY, slope=self.slope, rs=rs2,
                           y=pre_p, y_lo=pre_l, y_f32=pre_f, max_workgroups=max_wgs)
        else:
            mel_in = ws.plane("mel_in", rs2, self.odim, self.split)
            O.pack_rows(speech, None, mel_in, rs2)
            O.gemm(a=mel_in, b_ptr=wp.ptr, ldb=wp.ld, m=rs2.rows, n=C, act=L.ACT_LEAKY, slope=self.slope,
                   bias=self.mel_prenet[0].bias, rowmask_ptr=gap2.data_ptr(), out_f32_ptr=None if pre_f is None else pre_f.ptr,
                   ldo=C, out_plane=pre_p, out_plane_lo=pre_l, drop_p=pre_dp, drop_seed=pre_seed)
        return _Prenet(pre_f, pre_p, pre_l)

    def _mel_stack(self, st: _Pass, pre: _Prenet, rider=None) -> Plane:
        """mel encoder (+ mel_query_fc) (:162-164) -> q as the split-2 operand plane of q.k^T"""
        ws, pk, rs2, C = st.ws, st.pk, st.rs2, self.n_channels
        gap_ptr = st.gap2.data_ptr()
        if self.mel_query_fc is None:
            return self._res_stack(ws, "me", "mel_encoder", pk, rs2, pre.pre_f, pre.pre_p, gap_ptr, self.align_split, False, x_lo=pre.pre_l, rider=rider, drop=st.drop)[1]
        _, mh_p = self._res_stack(ws, "me", "mel_encoder", pk, rs2, pre.pre_f, pre.pre_p, gap_ptr, self.split, False, x_lo=pre.pre_l, rider=rider, drop=st.drop)
        q_p = ws.plane("q_p", rs2, C, self.align_split)
        wq = pk["qfc"]
        O.gemm(a=mh_p, b_ptr=wq.ptr, ldb=wq.ld, m=rs2.rows, n=C, bias=self.mel_query_fc.bias, rowmask_ptr=gap_ptr, out_plane=q_p)
        return q_p

    @staticmethod
    def _text_layers_alone(cur: _TextCursor, upto: int, plan) -> None:
        """the text-encoder layers in front of layer `upto`, each in an efts_resconv5 launch of its own under `plan` (:148)"""
        while cur.i < upto:
            O.resconv5(plan=plan, **cur.next())

    def _soft_index(self, st: _Pass, q_p: Plane, key_p: Plane, keep: bool):
        """scaled dot-product scores, softmax over the keys, expected key index per frame (:390-398, :168, :312)
        -> (sidx [B, T2], alpha [B, T1, T2] for keep, else None)"""
        ws, B, T1, T2, rs1, rs2, tl, ml, C = st.ws, st.B, st.T1, st.T2, st.rs1, st.rs2, st.tl, st.ml, self.n_channels
        sidx = ws.tensor("sidx", (B, T2))
        alpha = ws.tensor("alpha", (B, T1, T2)) if keep else None
        if T1 <= 128 and not keep and self.fuse_soft_index:
            # in one launch: a 128-column tile holds whole score rows, so the softmax over the keys and its expected index are taken
            # from the staged tile and the 4 B T2 T1 bytes of scores are neither written nor re-read
            O.gemm(a=q_p, b_ptr=key_p.ptr, ldb=key_p.ld, m=T2, n=T1, batch=B, a_batch_stride=rs2.Tp * q_p.ld,
                   b_batch_stride=rs1.Tp * key_p.ld, alpha=O.INV_SQRT(C), soft_index=sidx, key_len=tl, query_len=ml)
        else:
            scores = ws.tensor("scores", (B, T2, T1))                             # :390 q.k/sqrt(D)
            O.gemm(a=q_p, b_ptr=key_p.ptr, ldb=key_p.ld, m=T2, n=T1, batch=B, a_batch_stride=rs2.Tp * q_p.ld,
                   b_batch_stride=rs1.Tp * key_p.ld, alpha=O.INV_SQRT(C), out_f32_ptr=scores.data_ptr(), ldo=T1,
                   out_batch_stride=T2 * T1)
            O.attn_soft_index(scores, T1, tl, ml, sidx, alpha, B, T1, T2)         # :391-398, :168, :312
        return sidx, alpha

    def _imv(self, st: _Pass, sidx: torch.Tensor, alpha: Optional[torch.Tensor]) -> _Aligned:
        """index mapping vector, aligned positions e and the duration target log(delta e) (:314-345, :178-180, :203-216)"""
        ws, B, T1, T2, tl, ml = st.ws, st.B, st.T1, st.T2, st.tl, st.ml
        imv = torch.empty(B, T2, dtype=torch.float32, device=sidx.device)       # returned to the caller: written in place, no copy
        e, lde = ws.tensor("e", (B, T1)), ws.tensor("lde", (B, T1))
        if self.fuse_align and O.imv_align_fits(T1, T2):
            O.imv_align(sidx, tl, ml, float(self.sigma_e), float(self.duration_offset), self.delta_e_method_1, imv, e, lde, B, T1, T2)
        else:
            O.imv_scan(sidx, tl, ml, imv, B, T2)                                  # :314-323
            O.aligned_positions(imv, tl, ml, float(self.sigma_e), float(self.duration_offset), e, lde if self.delta_e_method_1 else None,
                                B, T1, T2)                                        # :178-180, :203-216
            if not self.delta_e_method_1:
                O.duration_target(e, tl, ml, float(self.duration_offset), False, lde, B, T1)   # :205-213
        return _Aligned(sidx, imv, e, lde, alpha)

    def _losses(self, st: _Pass, head: _Head, dur: torch.Tensor, lde: torch.Tensor) -> torch.Tensor:
        """(loss, mel_loss, duration_loss) on the device (:220-227), from the squared-error partials of the head's epilogue where it left them"""
        B, T1, T2, tl, ml = st.B, st.T1, st.T2, st.tl, st.ml
        out3 = torch.empty(3, dtype=torch.float32, device=ml.device)
        # use_masking=False (fastspeech_loss.py:63-67): plain means over the padded tensors = the masked sums taken with full lengths
        # (mel_pred, dur_pred and log_delta_e are zero beyond each item's length, speech is whatever the caller padded with)
        ml_loss = ml if self.use_masking else torch.full_like(ml, T2)
        tl_loss = tl if self.use_masking else torch.full_like(tl, T1)
        if head.sqerr_part is not None:
            O.losses_from_parts(head.sqerr_part, head.n_part, ml_loss, dur, lde, tl_loss, out3, B, T1, st.rs1.Tp, T2, self.odim)
        else:
            O.masked_losses(head.mel.data_ptr(), self.odim, st.speech, ml_loss, dur, lde, tl_loss, out3, st.ws.tensor("loss_ws", (1024,)), B, T1,
                            st.rs1.Tp, T2, T2, self.odim)
        return out3

    # ------------------------------------------------------------------ inference (efficient_tts.py:230-285)
    @torch.no_grad()
    def inference(self, text: torch.Tensor, text_lengths: torch.Tensor = None, *, length_scale: float = 1.0,
                  durations: Optional[torch.Tensor] = None, target_frames=None, return_durations: bool = False):
        """Free-running synthesis of ONE utterance: returns (mel_pred[1,T2,odim], reconst_alpha[1,T1,T2]).

        Duration control (keyword-only; the defaults are the reference's call): `length_scale` multiplies every duration (> 1:
        slower speech), `durations` [1, T1] (or [T1]) gives frames per phoneme -- entries >= 0 replace the prediction, negative
        ones keep it, the scale applies to both -- and `target_frames` rescales the utterance to exactly that many frames.
        return_durations=True appends the integer frames per phoneme [1, T1] int64 (they add up to T2).
        A call with any of these (return_durations=True alone included) runs as a ragged batch of one even with `graphs` off: that
        arithmetic masks every layer by the length and differs from the unmasked B = 1 pass of a plain graphs-off call by up to ~1e-4
        (with `graphs` on, the default, plain calls take that batched path too and the two agree bit for bit).  A total that does not
        fit an int32 frame count (a huge length_scale) is rejected with ValueError."""
        ctl = self._duration_controls(1, text.shape[-1], length_scale, durations, target_frames, return_durations)
        prev, self._free_running = self._free_running, True
        try:
            out = self._inference_impl(text, text_lengths, ctl)
        finally:
            self._free_running = prev
        return out if return_durations else out[:2]

    def _inference_impl(self, text: torch.Tensor, text_lengths: torch.Tensor = None, ctl=None):
        self._require(text)
        if text.shape[0] != 1:
            raise ValueError("inference() takes one utterance, like the reference (efficient_tts.py:361); "
                             "use inference_batch() for B > 1")
        if ctl is not None or (self.graphs and not torch.cuda.is_current_stream_capturing()):
            # same arithmetic as a ragged batch of one (every layer masked by the length; equal to the unmasked B = 1 pass
            # below to ~1e-4), on bucketed shapes whose launches replay as two hipGraphs around the one host sync
            # (text_lengths is accepted and ignored, like the reference's inference(): efficient_tts.py:233, :243 -- every position
            # of `text` is synthesised; ragged batches go through inference_batch())
            key = (text.device, text.shape[1])
            tl1 = self._len1.get(key)
            if tl1 is None:                                  # one int32 [T1] per length: no fill + cast launches per call
                if len(self._len1) > 4096:
                    self._len1.clear()
                tl1 = self._len1[key] = torch.full((1,), text.shape[1], dtype=torch.int32, device=text.device)
            if ctl is not None:                              # (with graphs off too: the controls live in the batched phase 1)
                mel, _, ralpha, frames = self._inference_batch_impl(text, None, None, tl_i32=tl1, want_lengths=False, ctl=ctl)
                return mel, ralpha, frames
            mel, _, ralpha = self._inference_batch_impl(text, None, None, tl_i32=tl1, want_lengths=False)
            return mel, ralpha
        dev = text.device
        T1, C = text.shape[1], self.n_channels
        pk = self.planes.get(self)
        ws = self._workspace(("inf", 1, T1), dev)
        rs1 = Rows(1, T1, self.row_gap)
        full = torch.full((1,), T1, dtype=torch.int32, device=dev)
        gap1 = ws.tensor("gap1", (rs1.rows,))
        O.row_masks(full, rs1, gap1, None)
        _, val_f, val_p = self._text_side(ws, pk, text.contiguous(), rs1, gap1, None)         # :246-255
        delta = self._duration(ws, pk, rs1, val_p, gap1, gap1.data_ptr(), 1)      # :258  clamp(exp(.)-offset, 0)
        e = ws.tensor("e", (1, T1))
        O.cumsum_rows(delta[:T1], e, 1, T1)                                       # :260
        t2 = int(torch.round(e[0, -1]).item())                                    # :361 (host sync, as the reference)
        if not self.delta_e_method_1:                                             # :261-265 + trim_e (:362-363): positions start at 0
            e = e - delta[:T1].view(1, T1)
        if t2 <= 0:
            raise ValueError("predicted total duration rounds to 0 frames")
        rs2 = Rows(1, t2, self.row_gap)
        ws2 = self._workspace(("inf2", 1, T1, t2), dev, pin=(ws,))
        gap2 = ws2.tensor("gap2", (rs2.rows,))
        O.row_masks(torch.full((1,), t2, dtype=torch.int32, device=dev), rs2, gap2, None)
        ralpha = torch.empty(1, T1, t2, dtype=torch.float32, device=dev)
        mel = self._expand_decode(ws2, pk, 1, T1, rs1, rs2, val_f, e, None, None, ralpha, None, gap2).mel   # :270-284
        return mel, ralpha

    # ------------------------------------------------------------------ batched ragged inference (extension)
    T1_BUCKET, T2_BUCKET = 16, 64       # free-running inference runs on shapes rounded up to these multiples (graph / workspace reuse)

    @staticmethod
    def _duration_controls(B: int, T1: int, length_scale, durations, target_frames, return_durations: bool):
        """Host-side checks of the duration controls of inference() / inference_batch(), before any device call.  None when no
        control is asked for (the calls of today, on their own graphs); else (scale [B] fp32, override [B, T1] fp32,
        target [B] int32), each None when absent and not yet on the device.  A length_scale of exactly 1.0 is no control."""
        scale = over = target = None
        if length_scale is not None:
            if isinstance(length_scale, torch.Tensor):
                if length_scale.dim() > 1 or length_scale.numel() not in (1, B):
                    raise ValueError(f"length_scale: a float or a [B] = [{B}] tensor, got shape {tuple(length_scale.shape)}")
                scale = length_scale.detach().reshape(-1).to(torch.float32).expand(B).contiguous()
                if not scale.is_cuda and not bool(((scale > 0) & torch.isfinite(scale)).all()):
                    raise ValueError("length_scale must be > 0 and finite")
            else:
                v = float(length_scale)
                if not (v > 0.0 and v != float("inf")):
                    raise ValueError(f"length_scale must be > 0 and finite, got {length_scale}")
                if v != 1.0:
                    scale = torch.full((B,), v, dtype=torch.float32)
        if durations is not None:
            d = torch.as_tensor(durations).detach()
            if B == 1 and d.dim() == 1:
                d = d[None]
            if tuple(d.shape) != (B, T1):
                raise ValueError(f"durations: [B, T1] = [{B}, {T1}] frames per phoneme (negative: predicted), got shape {tuple(d.shape)}")
            over = d.to(torch.float32).contiguous()
        if target_frames is not None:
            t = torch.as_tensor(target_frames).detach().reshape(-1)
            if t.numel() != B or t.is_floating_point() and not bool((t == t.round()).all()):
                raise ValueError(f"target_frames: {B} whole numbers of frames, got {tuple(torch.as_tensor(target_frames).shape)}")
            if not t.is_cuda and bool((t < 1).any()):
                raise ValueError("target_frames must be >= 1")
            target = t.to(torch.int32).contiguous()
        if scale is None and over is None and target is None and not return_durations:
            return None
        return scale, over, target

    def _infer_text(self, ws, text, tl, force_delta, ctl=None):
        """phase 1 (no host sync): embed -> text encoder -> value -> duration predictor -> aligned positions e = cumsum(durations)
        and the mel length of every item (efficient_tts.py:246-260).  text [B, T1] int64 (positions >= tl are ignored), tl int32 [B].
        ctl: device (scale, override, target) of the duration controls (any of them None): positions, lengths and the frames per
        phoneme from efts_duration_control, returned as a third output (mel length -1: a rejected item)."""
        dev = text.device
        B, T1 = text.shape
        pk = self.planes.get(self)
        rs1 = Rows(B, T1, self.row_gap)
        gap1, len1 = ws.tensor("gap1", (rs1.rows,)), ws.tensor("len1", (rs1.rows,))
        O.row_masks(tl, rs1, gap1, len1)
        # embedding with padded positions zeroed, then every layer masked by the item length
        h_p = self._text_stack(ws, pk, rs1, self._embed_text(ws, pk, text.contiguous(), rs1, tl, len1), len1.data_ptr())
        _, val_p = self._value_proj(ws, pk, rs1, h_p, len1, len1)                       # (:252-253)
        delta = self._duration(ws, pk, rs1, val_p, len1, len1.data_ptr(), 1)          # zero beyond each length
        # durations -> positions e = cumsum, mel lengths round(e[len - 1]) (:260, :270), positions from 0 for method 2 (:261-265)
        e = torch.empty(B, T1, dtype=torch.float32, device=dev)
        ml = torch.empty(B, dtype=torch.int32, device=dev)
        if ctl is None:
            O.duration_positions(delta, rs1.Tp, tl, force_delta, self.delta_e_method_1, e, ml, B, T1)
            return e, ml
        frames = torch.empty(B, T1, dtype=torch.int32, device=dev)
        O.duration_control(delta, rs1.Tp, tl, *ctl, self.delta_e_method_1, e, ml, frames, B, T1)
        return e, ml, frames

    def _infer_mel(self, ws, ws2, e, tl, ml, T2: int):
        """phase 2: Gaussian re-alignment from e, expand, decoder, mel head on a [B, T2] row space (efficient_tts.py:270-284);
        reads the value projection phase 1 left in `ws` (the (B, T1) workspace the caller holds: never looked up again by key,
        a pool eviction in between would hand back a fresh zero-filled one)."""
        dev = e.device
        B, T1 = e.shape
        C = self.n_channels
        pk = self.planes.get(self)
        rs1, rs2 = Rows(B, T1, self.row_gap), Rows(B, T2, self.row_gap)
        val_f = ws.f32("val_f", rs1, C)
        gap2, len2 = ws2.tensor("gap2", (rs2.rows,)), ws2.tensor("len2", (rs2.rows,))
        O.row_masks(ml, rs2, gap2, len2)
        ralpha = torch.empty(B, T1, T2, dtype=torch.float32, device=dev)
        mel = self._expand_decode(ws2, pk, B, T1, rs1, rs2, val_f, e, tl, ml, ralpha, len2.data_ptr(), len2).mel
        return mel, ralpha

    @torch.no_grad()
    def inference_batch(self, text: torch.Tensor, text_lengths: torch.Tensor, force_delta: Optional[float] = None, *,
                        length_scale=None, durations: Optional[torch.Tensor] = None, target_frames: Optional[torch.Tensor] = None,
                        return_durations: bool = False):
        """Free-running synthesis of B utterances at once -- an extension the reference cannot do
        (its inference() is B == 1 only: efficient_tts.py:361).  Every item is computed exactly as if it
        were alone: positions beyond an item's own length are kept at zero after EVERY layer (true
        zero padding, the opposite of the teacher-forced forward's leakage semantics), durations are
        accumulated per item and each item gets its own mel length T2_b = round(sum of durations).

        Returns (mel_pred [B, max T2_b, odim] zero-padded, mel_lengths [B] int64, reconst_alpha
        [B, T1, max T2_b]).  One host sync (max T2_b), like the reference's single `.item()`.

        With `graphs` on, the two phases run on bucketed shapes (T1 up to a multiple of 16, T2 of 64: padding is masked
        like any other ragged tail) and replay per-shape hipGraphs from the second call of a shape on.

        force_delta (benchmark hook): the duration predictor still runs, but every
        valid phoneme then gets this many frames, so a synthetic batch yields a known, equal T2.

        Duration control (keyword-only, as inference(); not together with force_delta): `length_scale` a float or a [B] tensor,
        `durations` [B, T1] frames per phoneme (negative: predicted), `target_frames` [B] exact mel lengths.  The controls are
        inputs of the phase-1 graph: a new pace replays it.  return_durations=True appends the frames per phoneme [B, T1] int64
        (0 beyond each text length; item b's add up to mel_lengths[b])."""
        ctl = self._duration_controls(text.shape[0], text.shape[1], length_scale, durations, target_frames, return_durations)
        if ctl is not None and force_delta is not None:
            raise ValueError("force_delta (benchmark hook) does not combine with length_scale / durations / target_frames / return_durations")
        prev, self._free_running = self._free_running, True
        try:
            out = self._inference_batch_impl(text, text_lengths, force_delta, ctl=ctl)
        finally:
            self._free_running = prev
        return out if return_durations else out[:3]

    def _inference_batch_impl(self, text, text_lengths, force_delta, tl_i32: Optional[torch.Tensor] = None, want_lengths: bool = True,
                              ctl=None):
        """tl_i32: the lengths already as an int32 device tensor (inference() keeps one per length); want_lengths=False: the caller
        drops the mel lengths (inference()), so they are not converted.  ctl: host-checked duration controls (_duration_controls):
        the frames per phoneme are returned as a fourth output"""
        self._require(text)
        with O.stream_scope():
            dev = text.device
            B, T1 = text.shape
            tl = tl_i32 if tl_i32 is not None else text_lengths.to(device=dev, dtype=torch.int32)
            graphs = self.graphs and not torch.cuda.is_current_stream_capturing()
            T1b = roundup(T1, self.T1_BUCKET) if graphs else T1
            self.planes.get(self)
            self._te0_table()                                 # (built outside the graphs, like the packed planes)
            wsig = (self.planes.tag(), self.opt.tag())
            ws = self._workspace(("infb", B, T1b), dev)
            if ctl is not None:
                ctl = tuple(None if c is None else c.to(dev) for c in ctl)
                have = tuple(c is not None for c in ctl)       # graph keys name the controls present, not their values
            frames = None
            if graphs and ctl is not None:
                def phase1c(t, l, *given):
                    it = iter(given)
                    with O.stream_scope():
                        return self._infer_text(ws, t, l, None, tuple(next(it) if h else None for h in have)) + (l,)
                ids = PadTo(text, (B, T1b)) if T1b != T1 else text.contiguous()
                given = [c if i != 1 or T1b == T1 else PadTo(c, (B, T1b)) for i, c in enumerate(ctl) if c is not None]
                e, ml, frames, tl = self._infer_cache.run(("text", B, T1b, "ctl", have), (ws.serial, wsig), (ids, tl, *given), phase1c,
                                                          keepalive=ws, clone=False)
            elif graphs:
                def phase1(t, l):
                    with O.stream_scope():              # resolved INSIDE the capture: the launches must go to the capturing stream
                        return self._infer_text(ws, t, l, force_delta) + (l,)
                # The graph's static outputs -- and its static copy of the lengths -- are handed on as they are: phase 2 reads them in
                # place (`refs`: no copies into inputs of its own; a re-captured phase 1 means new buffers, hence a new phase-2 capture).
                # The ids go straight into the zero-filled bucket-wide static input (positions beyond an item's length are ignored).
                ids = PadTo(text, (B, T1b)) if T1b != T1 else text.contiguous()
                e, ml, tl = self._infer_cache.run(("text", B, T1b, force_delta), (ws.serial, wsig), (ids, tl), phase1, keepalive=ws, clone=False)
            elif ctl is not None:
                e, ml, frames = self._infer_text(ws, text, tl, None, ctl)
            else:
                e, ml = self._infer_text(ws, text, tl, force_delta)
            if ctl is None:
                t2 = int((ml if B == 1 else ml.max()).item())                              # the one host sync
            else:
                mlh = ml.cpu()                                                             # the one host sync
                bad = (mlh < 0).nonzero().flatten().tolist()
                if bad:
                    raise ValueError(f"duration control rejected item(s) {bad}: length_scale must be > 0 and finite, target_frames >= 1 "
                                     "with a non-zero total duration, a total that fits an int32 frame count")
                t2 = int(mlh.max())
            if t2 <= 0:
                raise ValueError("predicted total durations round to 0 frames")
            T2b = roundup(t2, self.T2_BUCKET) if graphs else t2
            ws2 = self._workspace(("infb2", B, T1b, T2b), dev, pin=(ws,))
            if graphs:
                def phase2(e_, l, m):
                    with O.stream_scope():
                        return self._infer_mel(ws, ws2, e_, l, m, T2b)
                trim = T2b != t2 or T1b != T1
                mkey = ("mel", B, T1b, T2b) if ctl is None else ("mel", B, T1b, T2b, "ctl", have)   # (one phase 2 per phase-1 entry)
                mel, ralpha = self._infer_cache.run(mkey, (ws.serial, ws2.serial, wsig), (), phase2, keepalive=(ws, ws2),
                                                    refs=(e, tl, ml), clone=not trim)
                if trim:                                       # (the trimmed copies are the fresh tensors the caller gets)
                    # .clone(), not .contiguous(): at B == 1 (or t2 == T2b) the slice of the graph's static output is already
                    # contiguous and .contiguous() would hand the caller a VIEW the next call of this bucket overwrites
                    mel, ralpha = mel[:, :t2].clone(), ralpha[:, :T1, :t2].clone()
                if want_lengths:
                    ml = ml.to(torch.int64)                    # (a new tensor: `ml` is the text graph's static output)
            else:
                mel, ralpha = self._infer_mel(ws, ws2, e, tl, ml, T2b)
                ml = ml.to(torch.int64) if want_lengths else ml
            if ctl is not None:
                return mel, ml, ralpha, frames[:, :T1].to(torch.int64)       # (a new tensor: `frames` may be a graph's static output)
            return mel, ml, ralpha

    # ------------------------------------------------------------------ alignment of a recording (extension)
    @torch.no_grad()
    def align(self, text: torch.Tensor, text_lengths: torch.Tensor, speech: torch.Tensor, speech_lengths: torch.Tensor) -> dict:
        """Phoneme timings of recordings through the model's own teacher-forced alignment (efficient_tts.py:137-180, :203-213):
        the text side, the prenet, the mel encoder, the attention and the IMV -- the launches of forward() up to there, and
        nothing after them (no duration predictor, decoder, mel head or losses).  Dropout is never applied.  Returns a dict:
          e         [B, T1] fp32  the aligned positions forward() computes (:178-180);
          durations [B, T1] fp32  the reference's delta_e for this model's delta_e_method_1 (:203-213), 0 beyond each text length;
          frames    [B, T1] int64 the durations as whole frames (efts_duration_control: round(E_i) - round(E_{i-1}) of their
                                  cumulative sum E, so item b's add up to round(sum of its durations));
          imv       [B, T2] fp32  the index mapping vector (:174).
        `inference(text, durations=align(...)["durations"])` re-synthesises with the recorded timing."""
        self._require(text)
        B, T1 = text.shape
        with O.stream_scope():
            st, al = self._align_body(text, text_lengths, speech, speech_lengths)
            imv, tl, ml = al.imv, st.tl, st.ml
            e = al.e.clone()                               # (the workspace's buffer: the next forward() overwrites it)
            valid = torch.arange(T1, device=e.device)[None, :] < tl.to(torch.int64)[:, None]
            if self.delta_e_method_1:                      # :204  delta_e_i = e_i - e_{i-1}, e_{-1} = 0
                dur = torch.diff(e, dim=1, prepend=torch.zeros(B, 1, device=e.device))
            else:                                          # :205-213  delta_e_i = e_{i+1} - e_i with e_{len} = mel length
                ee = torch.cat([e, torch.zeros(B, 1, device=e.device)], dim=1)
                ee.scatter_(1, tl.to(torch.int64)[:, None], ml.to(torch.float32)[:, None])
                dur = ee[:, 1:] - ee[:, :-1]
            dur = torch.where(valid, dur, torch.zeros((), device=e.device))
            frames = torch.empty(B, T1, dtype=torch.int32, device=e.device)
            O.duration_control(dur, T1, tl, None, None, None, True, torch.empty_like(e), torch.empty_like(tl), frames, B, T1)
        return dict(e=e, durations=dur, frames=frames.to(torch.int64), imv=imv)


def _opt_property(name: str):
    def set_opt(self, v):
        v = type(getattr(LaunchOptions(), name))(v)
        if v and name in FP32_GENERIC_OPTIONS and self.split == L.SPLIT_FP32:
            raise ValueError(f"{name}=True: its fused kernel has no fp32 (operand format 3) form; a precision='fp32' model runs the generic path")
        setattr(self.opt, name, v)
    return property(lambda self: getattr(self.opt, name), set_opt)


for _f in dataclasses.fields(LaunchOptions):
    setattr(EfficientTTSCNN, _f.name, _opt_property(_f.name))
EfficientTTSCNN.RESCONV_MIN_ROWS = _opt_property("resconv_min_rows")      # (the names tests and tools of earlier rounds use)
EfficientTTSCNN.SMALL_M_ROWS = _opt_property("small_m_rows")
