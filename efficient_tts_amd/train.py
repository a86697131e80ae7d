"""Training step of EfficientTTSCNN on MI355X: forward with saved activations + hand-written
backward, all through the C ABI (reference: nntts/trainers/efficient_tts_trainer.py:139-160 calling
torch autograd on nntts/models/efficient_tts.py:120-228).

`TrainEngine.forward_backward()` returns the three losses and fills ONE flat fp32 gradient buffer
(views per parameter, laid out in backward-completion order so data-parallel buckets are contiguous
ranges that become final early: mel head + decoder first, text encoder + embedding last).
"""
from __future__ import annotations

import contextlib
from collections import namedtuple
from typing import Callable, Dict, List, Optional, Tuple

import torch

from . import lib as L
from . import ops as O
from .dropout import LAUNCH, DropoutPlan
from .ops import F32Rows, PackedWeight, Plane, Rows, hand_over
from .model import lengths_and_masks, require_trainable

# Test hooks and tuning constants of the training pass (module-level: bench.py --train-set NAME=INT, tests).  Round 6 removed the decided A/Bs
# (_PACK_SPLIT, _NARROW_TN, _EARLY_PACKS: always on) and did not keep its own (_WGRAD_EARLY, _TEXT_RIDERS, _HEAD_ORDER, _PACK_LATE,
# _WGRAD_GROUP_WGS_ME: all measured slower or equal, profiles/train_ab_r06.txt).  `switch_tag()` is what a captured step
# (step_graph.GraphedStep) is valid for.  Finished A/Bs of earlier rounds are no longer switches: the direct wgrad for taps 1 / 3
# (was _WGRAD_TN_SMALL) and the prenet through efts_frame_linear (was _FRAME_PRENET) are simply the code.
_WGRAD_TN_SPLITS = 8         # > 0: weight gradients on the direct (row-major, stream-K) kernel wherever its tiles fit; 0 = everything through the transposed
                             # planes + split-K efts_gemm (the path odd shapes always take: tests compare the two)
_SIGN_MIN_ROWS = 16384       # row spaces from here on: the forward convolutions of the stacks write the activation's sign words
                             # (efts_gemm `sign_mask`) and efts_act_bwd reads those instead of y and x in fp32 (14 -> 6 B per element);
                             # shorter ones (the text side) keep the narrow tiling, which does not write them.  0 = never
_BIAS_PARTS = 1              # direct-wgrad layers: bias gradient as per-row-block sums finished by the wgrad reduction (0: atomics in act_bwd; tests compare)
_RESCONV_FWD = 3             # residual stacks whose FORWARD runs on efts_resconv5 when their row space is long enough: bit 0 decoder,
                             # bit 1 mel encoder (A/B: bench.py --train-set _RESCONV_FWD=...)
_RESCONV_DGRAD = -1          # ... and whose DGRAD does (same bits as efts_gemm's); -1: decoder (bf16) / decoder + mel encoder (bf16x3), measured best:
                             # 3.72 -> 3.58-3.61 ms per B = 32 step with both switches (bf16), 6.96 -> 6.62-6.64 (bf16x3), tools/train_ab.sh
_WGRAD_WGS = 480             # split-K target: 480 workgroups per wgrad launch measured best (6.30 vs 6.60 ms/step at 640)
_WGRAD_STREAM = 3            # the mel-length weight gradients (mel head, decoder group, mel-encoder group, prenet) + their reductions on a third stream: nothing
                             # on the dgrad chain waits for them, and they fill what that chain leaves idle -- above all the backward of the alignment block,
                             # 0.25 ms of small latency-bound launches that use neither the matrix pipes nor the power budget.  Joined in front of a gradient
                             # bucket's hand-over (data parallel) or of the optimizer.  Bit 0: decoder group, bit 1: head, mel-encoder group, prenet (A/B)
_GV_ON_SIDE = 1              # eager steps: the dV branch of the alignment backward (pack_vt of dH + one batched product) on the text-side stream beside the d alpha' -> ... -> dK chain
                             # (3.51-3.63 -> 3.46-3.56 ms per step).  Captured into the step's hipGraph the extra branch costs 0.1 ms (3.41 vs 3.30 ms,
                             # bf16x3 6.55 vs 6.27: the replayed graph's stream assignment loses the overlap of the weight-gradient stream)
_FUSE_ACT_BWD = 1            # stacks whose dgrad runs on efts_resconv5: the activation backward of layer l - 1 in the epilogue of layer l's dgrad launch
                             # (csrc/efts_resconv_bwd.hip) instead of an efts_act_bwd launch of its own (0: separate launches; tests compare)
_WGRAD_GROUP_WGS = 384       # workgroups of a grouped launch (0: two per CU).  Swept 256..512 on the graphed B = 32 step: 3.27-3.32 ms at 384 against 3.33-3.34 at 512,
                             # 3.28-3.34 at 256 (per-layer launches: 3.48-3.50); the launch is bound by the chip, not by its busiest CU


def switch_tag() -> tuple:
    """every hook above, by value: part of the tag of a captured training step"""
    return (_WGRAD_TN_SPLITS, _SIGN_MIN_ROWS, _BIAS_PARTS, _RESCONV_FWD, _RESCONV_DGRAD, _WGRAD_WGS,
            _WGRAD_GROUP_WGS, _FUSE_ACT_BWD, O.RC_KERNEL, _WGRAD_STREAM)


class _TPlane(Plane):
    """transposed operand plane [channels][K = time] for wgrad"""

    def __init__(self, c: int, kpad: int, split: int, device):
        super().__init__(O.roundup(c, 128) + 136, kpad, split, device)
        self.c, self.kpad = c, kpad


class _TPlaneStack:
    """`n` transposed planes back to back (one per conv tap)"""

    def __init__(self, c: int, kpad: int, split: int, n: int, device):
        nrows = O.roundup(c, 128) + 136
        self.split = split
        self.nchunk = (kpad + O.chunk_k(split) - 1) // O.chunk_k(split)
        self.ld = self.nchunk * 128
        self.plane_bytes = nrows * self.ld
        self.buf = torch.zeros(n, nrows, self.ld, dtype=torch.uint8, device=device)
        self.ptr = self.buf.data_ptr()


def grad_layout(model) -> List[Tuple[str, torch.nn.Parameter]]:
    """Parameters in backward-completion order (see module docstring)."""
    named = dict(model.named_parameters())
    order: List[str] = []

    def conv(prefix):
        return [n for n in named if n.startswith(prefix)]

    order += conv("mel_output_layer.")
    for i in reversed(range(len(model.decoder.layers))):
        order += conv(f"decoder.layers.{i}.")
    order += conv("duration_predictor.")
    order += conv("mel_query_fc.")                       # (use_mel_query_fc: its gradient is ready in front of the mel encoder's)
    for i in reversed(range(len(model.mel_encoder.layers))):
        order += conv(f"mel_encoder.layers.{i}.")
    order += conv("mel_prenet.")
    order += conv("text_encoder_value.") + conv("text_encoder_key.")
    for i in reversed(range(len(model.text_encoder.layers))):
        order += conv(f"text_encoder.layers.{i}.")
    order += conv("text_embedding_table.")
    assert sorted(order) == sorted(named), "grad layout must cover every parameter exactly once"
    return [(n, named[n]) for n in order]


class _Step:
    """What every stage of one training step reads.  ws: the workspace of the shape; rs1 / rs2: text- and mel-length row spaces;
    gap* / len*: their row masks (0 on the gap rows / beyond each item's length as well); tl / ml: int32 lengths on the device;
    pk: packed forward planes by layer name (set by the repack); main / side / wst: the streams of the mel-length work, the
    text-length work (main itself without model.side_stream) and the mel-length weight gradients (None without _WGRAD_STREAM);
    drop: the step's Dropout masks (dropout.DropoutPlan: one mask per launch and step, regenerated by the backward from the same seed)"""
    __slots__ = ("ws", "text", "speech", "gscale", "B", "T1", "T2", "rs1", "rs2", "gap1", "len1", "gap2", "len2", "tl", "ml", "pk",
                 "main", "side", "wst", "drop")

    def __init__(self, **fields):
        self.pk = None
        for k, v in fields.items():
            setattr(self, k, v)


# What a stage hands to the stages behind it (`_f`: F32Rows, `_p`: operand Plane, `*_saved`: per-layer activations of _stack_fwd).
_StepOutputs = namedtuple("_StepOutputs", "imv ralpha mel")       # for the step's caller: workspace buffers, valid until the next step of the shape
_TextFwd = namedtuple("_TextFwd", "te_f te_p te_saved key_f key_p val_f val_p")
_DurFwd = namedtuple("_DurFwd", "h1_f l1_f l1_p h2_f dur")
_MelFwd = namedtuple("_MelFwd", "mel_in_f mel_in pre_f pre_z pre_drop mh_f mh_p q_f q_p me_saved")    # mh_*: only in front of a query fc
_AlignFwd = namedtuple("_AlignFwd", "scores sidx imv e lde ralpha ra_p h_f h_p")                               # ra_p: only where the expand is not fused
_DecFwd = namedtuple("_DecFwd", "d_f d_p dec_saved")
_LossFwd = namedtuple("_LossFwd", "out3 ml_loss tl_loss")
_LossBwd = namedtuple("_LossBwd", "dmel_f dmel_p ddur")
_Packs = namedtuple("_Packs", "val_p2 ra1_p kt qt")               # operands of the alignment backward that depend on forward tensors only
_DV = namedtuple("_DV", "GV GV_p")
_AlignBwd = namedtuple("_AlignBwd", "de dpi dsx dS GQ dSt")


class TrainEngine:
    def __init__(self, model):
        require_trainable(model, "TrainEngine")
        if len(model.duration_predictor.conv) != 2:
            # the step's duration-predictor stages (_fwd_duration, _bwd_duration) are written out for the two layers of the shipped recipe
            raise NotImplementedError(f"TrainEngine: n_duration_layer = {len(model.duration_predictor.conv)}: the training step implements "
                                      "the two-layer duration predictor only (synthesis runs any depth)")
        self.m = model
        self.layout = grad_layout(model)
        self.named = list(model.named_parameters())     # model.parameters() order (what autograd's Function receives)
        self.params = tuple(p for _, p in self.named)
        self.step_words = None                          # device uint32[8], set while a step is captured / replayed as a hipGraph
                                                        # (step_graph.GraphedStep).  This engine reads word 3 alone, 2 * dropout step; the rest are
                                                        # the optimizer's float bits: words 0-2 {lr, 1 - b1^t, sqrt(1 - b2^t)} of efts_adam_amsgrad_dev,
                                                        # words 4-7 those of efts_optim_hyper, whichever kernel the optimizer runs (the others stay 0)
        self.step_params = None                         # tuple(model.parameters()) of the running step (autograd.py), saves re-walks
        self.dev = next(model.parameters()).device
        self.numel = sum(p.numel() for _, p in self.layout)
        pad = (-self.numel) % 4
        self.flat = torch.zeros(self.numel + pad, dtype=torch.float32, device=self.dev)
        self.g: Dict[str, torch.Tensor] = {}
        self.offsets: Dict[str, Tuple[int, int]] = {}
        off = 0
        for n, p in self.layout:
            self.g[n] = self.flat[off:off + p.numel()].view_as(p)
            self.offsets[n] = (off, off + p.numel())
            off += p.numel()
        # bucket boundaries (element offsets into `flat`): head+decoder | dur+mel side | text side
        self.bucket_ends = [self.offsets[[n for n, _ in self.layout if n.startswith("decoder.layers.0.")][-1]][1],
                            self.offsets[[n for n, _ in self.layout if n.startswith("mel_prenet.")][-1]][1],
                            self.numel]
        self.folded: Dict[str, torch.Tensor] = {}
        self.wt: Dict[str, PackedWeight] = {}
        self._ws_tag = ""                       # "s" while work is being enqueued on the side stream
        self.bucket_hook: Optional[Callable[[int], None]] = None
        self.join_reduce: Optional[Callable[[], None]] = None
        self.mark: Optional[Callable[[str], None]] = None      # timing probe of the data-parallel wrapper (bench only)
        self.last: Optional[_StepOutputs] = None               # outputs of the last step (set by forward_backward)
        self.bound = set()                      # who holds views of `flat` (EftsAdam, DistributedEFTS): see autograd.engine_of

    def stale(self, model) -> bool:
        """True when the model's parameter set no longer matches the layout captured at construction
        (remove_weight_norm / apply_weight_norm / .to(device))."""
        cur = {n: p for n, p in model.named_parameters()}
        return set(cur) != set(self.g) or any(cur[n].shape != self.g[n].shape or cur[n].device != self.dev for n in cur)

    # ------------------------------------------------------------------ weights for the backward
    @staticmethod
    def _pack_phase(name: str) -> str:
        """the phase of the training step's repack a weight's planes (forward and dgrad in one pass) belong to: "te" on the text stream (text
        encoder, duration predictor, key / value), "me" on the main one.  A finer split measured slower in round 6: 3.23 -> 3.25-3.27 ms (bf16),
        5.93-5.97 -> 6.02-6.05 (bf16x3) under bench.py's clock (profiles/train_ab_r06.txt)."""
        return "te" if name.startswith(("text_encoder.", "dur.", "key", "value")) else "me"

    def _prepare_weights(self):
        """schedules the repack of the forward planes, folded fp32 weights and transposed / flipped dgrad planes (WeightPlanes.schedule)"""
        m = self.m
        for name, mod, cout, cin, taps in m.planes.modules(m):
            if name not in self.wt and name != "prenet":          # (the prenet's input is the frames: no dgrad plane)
                if hasattr(mod, "weight_g") and (cout % 64 or cin % 64 or taps > 5):
                    self.folded[name] = torch.empty(cout, cin, taps, device=self.dev)   # row-kernel shapes only
                self.wt[name] = PackedWeight(cin, cout, taps, m.split, self.dev)
        return m.planes.schedule(m, self.folded, self.wt, self.step_params, self._pack_phase)

    # ------------------------------------------------------------------ small wrappers
    def _wgrad_any(self, ws, dz_f_ptr, dz_p: Optional[Plane], x_f_ptr, x_p: Optional[Plane], cout, cin, taps, rows, out_dw, defer: Optional[list] = None):
        """un-normed weights: the direct kernel when both operand planes exist in one format and the shape fits its tiles.
        defer: a list that collects the direct items of equally shaped layers for ONE grouped launch (the caller passes it to
        _wgrad_group once the operand planes of all of them are final and still intact)"""
        if (_WGRAD_TN_SPLITS > 0 and dz_p is not None and x_p is not None and dz_p.split == x_p.split
                and cout % 128 == 0 and cin % 64 == 0 and taps in (1, 3, 5)):
            item = (dz_p, x_p, None, None, out_dw, None, None, None)
            if defer is not None:
                defer.append(item)
            else:
                self._wgrad_group(ws, [item], cout, cin, rows, taps, dz_p.split)
        else:
            self._wgrad(ws, dz_f_ptr, cout, x_f_ptr, cin, cin, taps, rows, None, None, out_dw, None)

    def _wgrad(self, ws, dz_ptr, cout, x_ptr, ldx, cin, taps, rows, v, g, out_dw, out_dg):
        """dW[co][ci][k] = sum_t dZ[t][co] X[t+k-pad][ci] as `taps` split-K GEMMs on transposed planes"""
        split = self.m.split
        ck = O.chunk_k(split)
        tiles = ((cout + 127) // 128) * ((cin + 127) // 128)
        nch_total = (rows + ck - 1) // ck
        S = max(1, min(32, (_WGRAD_WGS + tiles * taps - 1) // (tiles * taps), nch_total))    # ~_WGRAD_WGS workgroups per launch
        nch = (nch_total + S - 1) // S
        kpad = O.roundup(S * nch * ck, 64)
        tag = self._ws_tag                       # the side stream owns its own scratch (both streams run wgrads at once)
        zt = ws.get(("zt", tag, cout, kpad, split), lambda: _TPlane(cout, kpad, split, self.dev))
        O.pack_t(dz_ptr, cout, zt, rows, cout, kpad)
        part = ws.get(("part", tag, taps, S, cout, cin), lambda: torch.empty(taps, S, cout, cin, device=self.dev))
        pad = (taps - 1) // 2
        xts = ws.get(("xt", tag, cin, kpad, split, taps), lambda: _TPlaneStack(cin, kpad, split, taps, self.dev))
        O.pack_t(x_ptr, ldx, xts, rows, cin, kpad, shift=-pad, taps=taps, tap_stride=xts.plane_bytes)
        O.gemm(a=zt, b_ptr=xts.ptr, ldb=xts.ld, m=cout, n=cin, batch=S, nchunk=nch, a_batch_stride=nch * 128, b_batch_stride=nch * 128,
               out_f32_ptr=part.data_ptr(), ldo=cin, out_batch_stride=cout * cin, batch2=taps, b_batch2_stride=xts.plane_bytes,
               out_batch2_stride=S * cout * cin)
        O.wgrad_reduce(part, S, v, g, out_dw, out_dg, cout, cin, taps)

    def _wgrad_group(self, ws, items, cout, cin, rows, taps: int, split: int, wgs: Optional[int] = None):
        """the direct weight gradients of several layers of one stack (same shape, same row space) as ONE stream-K launch and ONE
        reduction (csrc/efts_wgrad.hip `wgrad_sk_kernel`, csrc/efts_train.hip `wgrad_reduce_sk_kernel`).
        items: (dz_p, x_p, v, g, out_dw, out_dg, bias_part, dbias) per layer (more than the library takes per launch: several launches)"""
        if len(items) > L.WGRAD_MAX_ITEMS:
            for i in range(0, len(items), L.WGRAD_MAX_ITEMS):
                self._wgrad_group(ws, items[i:i + L.WGRAD_MAX_ITEMS], cout, cin, rows, taps, split, wgs)
            return
        n, wgs = len(items), _WGRAD_GROUP_WGS if not wgs else wgs
        key = ("gpart", self._ws_tag, n, rows, cout, cin, taps, split, wgs)
        O.wgrad_grouped(items, rows, cout, cin, taps, split, wgs, lambda nbytes: ws.get(key, lambda: torch.empty(nbytes // 4, device=self.dev)))

    @staticmethod
    def _narrow_ok(dz_split: int, x_split: int, cout: int, cin: int, ldz: int, ldx: int) -> bool:
        """THE applicability test of _wgrad_narrow (callers that allocate differently for the two paths ask this, not a copy of it)"""
        return bool(_WGRAD_TN_SPLITS > 0 and dz_split == 1 and x_split == 1 and max(cout, cin) % 128 == 0 and min(cout, cin) <= 128
                    and ldz >= max(cout, 128) * 2 and ldx >= max(cin, 128) * 2)

    def _wgrad_narrow(self, ws, tag, dz_p: Plane, x_p: Plane, cout, cin, rows, out_dw) -> bool:
        """weight gradient of a Linear with an 80-channel side (mel head 512 -> 80, prenet 80 -> 512) on the direct kernel: bf16 planes are
        128 columns wide (two 64-channel chunks, zeros beyond the 80th), so the contraction runs on the padded 128 and the result's first
        80 rows / columns are copied out -- instead of two transposed operand copies (efts_pack_t over the mel-length stream) + split-K
        efts_gemm + reduction.  False: not applicable (bf16x3 planes are 96 wide), the caller takes the transposed-plane path."""
        if not self._narrow_ok(dz_p.split, x_p.split, cout, cin, dz_p.ld, x_p.ld):
            return False
        co_p, ci_p = max(cout, 128), max(cin, 128)
        scratch = ws.tensor(f"B{tag}_dw_pad", (co_p, ci_p))
        self._wgrad_group(ws, [(dz_p, x_p, None, None, scratch, None, None, None)], co_p, ci_p, rows, 1, 1)     # 8 tiles, stream-K over the rows
        out_dw.copy_(scratch[:cout, :cin])
        return True

    # ------------------------------------------------------------------ forward with saved activations
    def _stack_fwd(self, ws, tag, blk, pk, rs, x_f, x_p, gap_ptr, last_split, drop: DropoutPlan):
        m, C = self.m, self.m.n_channels
        saved = []
        layers = getattr(m, blk).layers
        if (_RESCONV_FWD & dict(dec=1, me=2, te=0)[tag]) and m._on_resconv(rs, drop) and _WGRAD_TN_SPLITS > 0 and C % 128 == 0:
            # mel-length stack on efts_resconv5 (the inference kernel): the stream between the layers is hi + lo bf16 planes (every
            # hi plane is kept: it is the layer's operand in the wgrad), the activation's sign leaves the epilogue as bit rows
            # (efts_act_bwd mode 5); fp32 only into the first layer (the producer's stream) and out of the last one
            n = len(layers)
            x_lo = None
            for i, layer in enumerate(layers):
                last = i == n - 1
                o_split = last_split if last else m.split
                o_p = ws.plane(f"T{tag}_p{i}", rs, C, o_split)
                o_l = ws.plane(f"T{tag}_l{i & 1}", rs, C, 1) if (o_split == 1 and not last) else None
                o_f = ws.f32(f"T{tag}_f{n - 1}", rs, C) if last else None
                sg = ws.tensor(f"T{tag}_sb{i}", (rs.rows, C // 8), torch.uint8)
                O.resconv5(x=x_p, x_lo=x_lo, x_f32_ptr=x_f.ptr if i == 0 else None, ldr=C, w=pk[f"{blk}.{i}"], taps=m.k_size, m=rs.rows, n=C,
                           bias=layer.conv[0].bias, slope=m.slope, rowmask_ptr=gap_ptr, y_f32_ptr=None if o_f is None else o_f.ptr, ldo=C,
                           y=o_p, y_lo=o_l, sign_bits_ptr=sg.data_ptr())
                saved.append((None, None, x_p, (sg, 5), 0.0, 0))
                x_p, x_lo = o_p, o_l
            return o_f, x_p, saved
        for i, layer in enumerate(layers):
            last = i == len(layers) - 1
            w = pk[f"{blk}.{i}"]
            o_f = ws.f32(f"T{tag}_f{i}", rs, C)
            o_p = ws.plane(f"T{tag}_p{i}", rs, C, last_split if last else m.split)
            dp, dseed = drop.conv(LAUNCH[tag] + i)
            if m.act_general is not None:
                # a torch.nn activation outside the contraction epilogues (csrc/efts_act.hip): the pre-activation is kept in fp32 for f'(z)
                z = ws.f32(f"T{tag}_z{i}", rs, C)
                O.gemm(a=x_p, b_ptr=w.ptr, ldb=w.ld, b_tap_stride=w.tap_stride, taps=m.k_size, m=rs.rows, n=C, bias=layer.conv[0].bias,
                       out_f32_ptr=z.ptr, ldo=C)
                O.act_apply(m.act_general, z.ptr, x_f.ptr, gap_ptr, o_f, o_p, rs.rows, C, dp, dseed)
                saved.append((x_f, o_f, x_p, (z, "z"), dp, dseed))
                x_f, x_p = o_f, o_p
                continue
            # under Dropout y - x no longer carries the activation's sign where the element was dropped: always the sign words then
            sg = ws.tensor(f"T{tag}_sg{i}", (rs.rows, C // 8), torch.uint8) if ((0 < _SIGN_MIN_ROWS <= rs.rows or dp > 0) and C % 128 == 0) else None
            O.gemm(a=x_p, b_ptr=w.ptr, ldb=w.ld, b_tap_stride=w.tap_stride, taps=m.k_size, m=rs.rows, n=C, act=L.ACT_LEAKY, slope=m.slope,
                   bias=layer.conv[0].bias, resid_ptr=x_f.ptr, ldr=C, rowmask_ptr=gap_ptr, out_f32_ptr=o_f.ptr, ldo=C, out_plane=o_p,
                   sign_mask_ptr=None if sg is None else sg.data_ptr(), drop_p=dp, drop_seed=dseed)
            saved.append((x_f, o_f, x_p, None if sg is None else (sg, 4), dp, dseed))
            x_f, x_p = o_f, o_p
        return x_f, x_p, saved

    @contextlib.contextmanager
    def _forked(self, st):
        """launches of the body go to stream `st`, ordered behind everything already enqueued on the current stream (None: no-op)"""
        if st is None:
            yield
            return
        hand_over(torch.cuda.current_stream(self.dev), st)
        with self._on(st, "w"):                 # (scratch of its own: the other streams run weight gradients at the same time)
            yield

    @contextlib.contextmanager
    def _on(self, st, tag: str = "s"):
        """launches of the body go to stream `st` and take their scratch from the namespace `tag` ("s": the text-side stream, which
        runs weight gradients at the same time as the main one)"""
        keep_tag = self._ws_tag
        with O.on_stream(st):
            self._ws_tag = tag
            try:
                yield
            finally:
                self._ws_tag = keep_tag

    def _stack_bwd(self, ws, tag, blk, rs, G: F32Rows, saved, gap_ptr, final_mask_ptr, final_plane: Optional[Plane], wgrad_stream=None):
        """backward through n x (x + leaky(conv(x))); returns the gradient w.r.t. the stack input.
        wgrad_stream: the stack's grouped weight gradients (and their reduction) are enqueued there, behind an event of the current stream
        (their operands -- every layer's dZ plane and input plane -- are final then and not written again in this step); the caller joins"""
        m, C = self.m, self.m.n_channels
        layers = getattr(m, blk).layers
        group = []                                               # (grouped direct wgrads: every layer keeps its dZ plane and bias sums until the stack is through)
        on_rc = bool((_RESCONV_DGRAD if _RESCONV_DGRAD >= 0 else (1 if m.split == 1 else 3)) & dict(dec=1, me=2, te=0)[tag]) and m._on_resconv(rs)
        fused = None                                             # (dZ plane, bias sums) of layer i the dgrad launch of layer i + 1 has already written
        for i in reversed(range(len(layers))):
            x_f, y_f, x_pl, sg, dp, dseed = saved[i]
            conv = layers[i].conv[0]
            pre = f"{blk}.layers.{i}.conv.0."
            direct = _WGRAD_TN_SPLITS > 0 and C % 128 == 0 and x_pl.split == m.split and m.k_size <= 5     # (efts_wgrad_tn_grouped: taps 1 / 3 / 5)
            keep = str(i) if direct else ""
            if fused is not None:
                dz_p, bp = fused
                dz_f = None
            else:
                dz_p = ws.plane(f"B{tag}_dzp{keep}", rs, C, m.split)
                # the direct wgrad and the dgrad both read dZ as the bf16 plane: its fp32 copy is only written for the
                # transposed-plane path
                dz_f = None if direct else ws.f32(f"B{tag}_dz", rs, C)
                # direct path: the bias gradient leaves act_bwd as per-row-block sums and is finished by the wgrad reduction
                # (no same-address atomics: ~8 of 22 us per launch at mel length)
                bp = ws.tensor(f"B{tag}_bp{keep}", ((rs.rows + 63) // 64, C)) if (direct and _BIAS_PARTS) else None
                db, parts = (bp, L.ACT_BWD_BIAS_PARTS) if bp is not None else (self.g[pre + "bias"], 0)
                if sg is not None and sg[1] == "z":                  # general activation: f'(z) from the kept pre-activation, bias gradient by atomics
                    bp = None
                    O.act_grad(m.act_general, G.ptr, sg[0].ptr, gap_ptr, dz_f, dz_p, self.g[pre + "bias"], rs.rows, C, dp, dseed)
                elif sg is not None:                                 # (sign words of efts_gemm: mode 4; sign bits of efts_resconv5: mode 5)
                    O.act_bwd_dropout(G.ptr, sg[0].data_ptr(), None, gap_ptr, m.slope, sg[1] | parts, dz_f, dz_p, db, rs.rows, C, dp, dseed)
                else:
                    O.act_bwd_dropout(G.ptr, y_f.ptr, x_f.ptr, gap_ptr, m.slope, 1 | parts, dz_f, dz_p, db, rs.rows, C, dp, dseed)
            wn = hasattr(conv, "weight_g")
            v_, g_ = (conv.weight_v.detach(), conv.weight_g.detach()) if wn else (None, None)
            dw_, dg_ = (self.g[pre + "weight_v"], self.g[pre + "weight_g"]) if wn else (self.g[pre + "weight"], None)
            if direct:
                group.append((dz_p, x_pl, v_, g_, dw_, dg_, bp, self.g[pre + "bias"]))
            else:
                self._wgrad(ws, dz_f.ptr, C, x_f.ptr, C, C, m.k_size, rs.rows, v_, g_, dw_, dg_)
            wt = self.wt[f"{blk}.{i}"]
            Gn = ws.f32(f"B{tag}_G{i & 1}", rs, C)
            last = i == 0
            fused = None
            if on_rc and dz_p.split == m.split:
                # dgrad on the persistent kernel: G' = (G + conv_T(dZ)) * mask = a residual layer with the transposed weights, no bias
                # and slope 1, fp32 gradient stream in and out (bit-identical to the efts_gemm launch)
                below = saved[i - 1] if i > 0 else None
                if (_FUSE_ACT_BWD and below is not None and below[3] is not None and below[3][1] == 5 and below[4] == 0.0 and direct
                        and _BIAS_PARTS and m.k_size == 5 and below[2].split == m.split):
                    # ... and the activation backward of layer i - 1 on G' while the epilogue holds it: dZ_{i-1} as its operand plane and one
                    # row of column sums per tile (the launch efts_act_bwd would otherwise read G' back for)
                    nz_p = ws.plane(f"B{tag}_dzp{i - 1}", rs, C, m.split)
                    nbp = ws.tensor(f"B{tag}_bq{i - 1}", (O.resconv5_bias_rows(rs.rows, C), C))
                    O.resconv5(x=dz_p, x_f32_ptr=G.ptr, ldr=C, w=wt, taps=5, m=rs.rows, n=C, slope=1.0, rowmask_ptr=gap_ptr, y_f32_ptr=Gn.ptr, ldo=C,
                               y=nz_p, act_bwd_sign_ptr=below[3][0].data_ptr(), act_bwd_slope=m.slope, act_bwd_bias_part=nbp)
                    fused = (nz_p, nbp)
                else:
                    O.resconv5(x=dz_p, x_f32_ptr=G.ptr, ldr=C, w=wt, taps=m.k_size, m=rs.rows, n=C, slope=1.0,
                               rowmask_ptr=final_mask_ptr if last else gap_ptr, y_f32_ptr=Gn.ptr, ldo=C, y=final_plane if last else None)
            else:
                O.gemm(a=dz_p, b_ptr=wt.ptr, ldb=wt.ld, b_tap_stride=wt.tap_stride, taps=m.k_size, m=rs.rows, n=C, resid_ptr=G.ptr, ldr=C,
                       rowmask_ptr=final_mask_ptr if last else gap_ptr, out_f32_ptr=Gn.ptr, ldo=C,
                       out_plane=final_plane if last else None)
            G = Gn
        if group:
            with self._forked(wgrad_stream):
                self._wgrad_group(ws, group, C, C, rs.rows, m.k_size, m.split)
        return G

    def forward_backward(self, text, text_lengths, speech, speech_lengths, gscale: Optional[torch.Tensor] = None,
                         keep: bool = False):
        """One fwd+bwd.  Returns (out3 = [loss, mel_loss, dur_loss] device tensor, aux dict)."""
        with O.stream_scope():
            return self._forward_backward(text, text_lengths, speech, speech_lengths, gscale, keep)

    def _mark(self, name: str):
        if self.mark is not None:
            self.mark(name)

    def _forward_backward(self, text, text_lengths, speech, speech_lengths, gscale, keep):
        """The schedule of the step: every stage call, stream fork and join, bucket hand-over and timing mark, in order.  Its only
        device work of its own is the repack's two phases and the zeroing of the gradient buffer; every other launch is in a stage.
        Three HIP streams.  The text-length work (embedding, text encoder, K/V, duration predictor and all of their backward) runs on
        ~B*T1 = 4k rows: launches of 70-270 workgroups that leave most of the chip idle.  None of it depends on the mel-length work
        except through K/V (forward) and dK/dV/d(dur) (backward), so it goes to the `side` stream and fills the idle CUs / tail rounds
        of the mel-length kernels on `main`.  The mel-length weight gradients go to `wst` (the stages' `wgrad_stream`, forked inside them
        by _forked behind their operands; joined here)."""
        m = self.m
        L.require_device()
        st = self._begin_step(text, text_lengths, speech, speech_lengths, gscale)       # masks on main
        main, side, wst = st.main, st.side, st.wst
        wst2 = wst if (_WGRAD_STREAM & 2) else None
        # the repack of the operand planes (weight-norm fold + bf16 planes + dgrad planes, ~110 us on one stream): the text-side planes on
        # the stream the text side runs on, the mel-side planes here -- both behind the masks and the previous step's optimizer
        side.wait_stream(main)
        st.pk = self._prepare_weights()
        m.planes.issue("me")
        with self._on(side):
            m.planes.issue("te")
        self.flat.zero_()
        self._mark("step_start")

        # ============================ forward (efficient_tts.py:144-227), activations kept
        with self._on(side):
            tx = self._fwd_text(st)
            ev_kv = hand_over(side)
            du = self._fwd_duration(st, tx)                          # needs V only
            ev_dur = hand_over(side)
        mf = self._fwd_mel(st)
        self._mark("fwd_mel_encoder_done")
        main.wait_event(ev_kv)                                      # K, V from the side stream, behind the mel encoder
        al = self._fwd_alignment(st, mf, tx)
        self._mark("fwd_alignment_done")
        dec = self._fwd_expand_decoder(st, al, tx)
        self._mark("fwd_decoder_done")
        mel = self._fwd_head(st, dec)
        main.wait_event(ev_dur)                                     # predicted durations from the side stream
        lo = self._fwd_losses(st, mel, du, al)
        self.last = _StepOutputs(al.imv, al.ralpha, mel)

        # ============================ backward
        self._mark("backward_start")
        lb = self._bwd_loss(st, mel, du, al, lo)
        hand_over(main, side)                                       # d(dur) is ready
        with self._on(side):
            dV_dur = self._bwd_duration(st, du, tx, lb)
            ev_durb = hand_over(side)
            pa = self._bwd_operand_packs(st, tx, mf, al)
            ev_packs = hand_over(side)
        dH, dH_p = self._bwd_head_decoder(st, lb, dec, wst2, wst if (_WGRAD_STREAM & 1) else None)
        self._mark("bwd_decoder_done")
        if self.bucket_hook and wst is None:
            self.bucket_hook(0)
        main.wait_event(ev_packs)
        dAp, dHt, dv = self._bwd_dalpha(st, pa, dH_p)                 # dv: buffers only (allocated here to keep the order); _bwd_dv fills them
        ev_gv = None
        if _GV_ON_SIDE and m.side_stream and not torch.cuda.is_current_stream_capturing():
            # nothing between here and dK reads dV: the branch runs on the text-side stream (idle until dK / dV exist, and the consumer of
            # both) beside the chain d alpha' -> ... -> dQ, dK instead of in front of it; a capturing pass keeps it here (see _GV_ON_SIDE)
            hand_over(main, side)                                    # dH
            with self._on(side):
                self._bwd_dv(st, dH, dHt, pa, dV_dur, dv)            # (dV_dur and alpha' as an operand were produced on this stream)
                ev_gv = hand_over(side)
        else:
            main.wait_event(ev_durb)                                 # dV of the duration predictor (and its gradients: bucket 1)
            self._bwd_dv(st, dH, dHt, pa, dV_dur, dv)
        ab = self._bwd_alignment(st, al, dAp, pa)
        if ev_gv is not None:
            main.wait_event(ev_gv)                                   # (shared: dV is the residual of the next launch; else: one join for everything behind)
        GK, GK_p = self._bwd_dk(st, ab, pa, dv)
        ev_gk = hand_over(main)
        self._mark("bwd_alignment_done")
        side.wait_event(ev_gk)                                      # dK, dV are ready
        if wst is not None and self.bucket_hook:
            # data parallel: bucket 0 (mel head + decoder) is final once the decoder's weight gradients are through; its exchange then
            # overlaps the encoders' backward instead of the alignment block's as well
            main.wait_stream(wst)
            self.bucket_hook(0)
        with self._on(side):
            Ge = self._bwd_text(st, tx, dv, GK, GK_p)
        Gm = self._bwd_mel_encoder(st, mf, ab.GQ, wst2)
        self._mark("bwd_mel_encoder_done")
        self._bwd_prenet(st, mf, Gm, wst2)
        if self.bucket_hook:
            if wst is not None:
                main.wait_stream(wst)
            self.bucket_hook(1)
        main.wait_stream(side)                                      # text-side gradients (bucket 2) and everything else enqueued there
        if wst is not None and not self.bucket_hook:
            main.wait_stream(wst)                                   # the weight gradients of the mel-length layers
        if self.bucket_hook:
            self.bucket_hook(2)
        aux = None
        if keep:
            aux = dict(imv=al.imv, ralpha=al.ralpha, mel=mel, e=al.e, dH=dH, dAp=dAp, de=ab.de, dpi=ab.dpi, dsx=ab.dsx, dS=ab.dS, GQ=ab.GQ,
                       GK=GK, GV=dv.GV, Gm=Gm, Ge=Ge, rs1=st.rs1, rs2=st.rs2, ddur=lb.ddur)
        return lo.out3, aux

    # ------------------------------------------------------------------ the stages of the step (launches; no join, and no fork but _forked to the `wgrad_stream` a stage is given)
    def _begin_step(self, text, text_lengths, speech, speech_lengths, gscale) -> _Step:
        """workspace, row spaces, masks (launched on the current stream), streams and the step's Dropout words"""
        m, dev = self.m, self.dev
        B, T1 = text.shape
        T2 = speech.shape[1]
        text, speech = text.contiguous(), speech.contiguous().float()
        ws = m._workspace(("train", B, T1, T2), dev)
        rs1, rs2 = Rows(B, T1, m.row_gap), Rows(B, T2, m.row_gap)
        gap1, len1 = ws.tensor("gap1", (rs1.rows,)), ws.tensor("len1", (rs1.rows,))
        gap2, len2 = ws.tensor("gap2", (rs2.rows,)), ws.tensor("len2", (rs2.rows,))
        tl, ml, masks_done = lengths_and_masks(text_lengths, speech_lengths, dev, rs1, rs2, gap1, len1, gap2, len2)
        if not masks_done:
            O.row_masks(tl, rs1, gap1, len1)
            O.row_masks(ml, rs2, gap2, len2)
        # the next step of the mask sequence; one that is being captured (step_graph.GraphedStep) adds device word 3 of `step_words` to its duration seeds
        drop = m.step_dropout(None if self.step_words is None else self.step_words.data_ptr() + 12)
        return _Step(ws=ws, text=text, speech=speech, gscale=gscale, B=B, T1=T1, T2=T2, rs1=rs1, rs2=rs2,
                     gap1=gap1, len1=len1, gap2=gap2, len2=len2, tl=tl, ml=ml, main=torch.cuda.current_stream(dev), side=m._side_stream(dev),
                     wst=m._aux_stream(dev) if (_WGRAD_STREAM and m.side_stream) else None, drop=drop)

    def _fwd_text(self, st: _Step) -> _TextFwd:
        """embedding, text encoder, key / value Linears"""
        m, ws, rs1, C, split = self.m, st.ws, st.rs1, self.m.n_channels, self.m.split
        emb_f, emb_p = ws.f32("Temb_f", rs1, C), ws.plane("Temb_p", rs1, C, split)
        O.embed(st.text, m.text_embedding_table.weight.detach(), emb_f, emb_p, rs1)
        te_f, te_p, te_saved = self._stack_fwd(ws, "te", "text_encoder", st.pk, rs1, emb_f, emb_p, st.gap1.data_ptr(), split, st.drop)
        key_f, key_p = ws.f32("Tkey_f", rs1, C), ws.plane("Tkey_p", rs1, C, 2)
        val_f, val_p = ws.f32("Tval_f", rs1, C), ws.plane("Tval_p", rs1, C, split)
        shared = m.share_text_encoder_key_value                 # efficient_tts.py:150-153: the value is the key projection
        wk = st.pk["key"]
        wv = wk if shared else st.pk["value"]
        O.gemm(a=te_p, b_ptr=wk.ptr, ldb=wk.ld, m=rs1.rows, n=C, bias=m.text_encoder_key.bias, rowmask_ptr=st.len1.data_ptr(),
               out_f32_ptr=key_f.ptr, ldo=C, out_plane=key_p)
        O.gemm(a=te_p, b_ptr=wv.ptr, ldb=wv.ld, m=rs1.rows, n=C, bias=(m.text_encoder_key if shared else m.text_encoder_value).bias,
               rowmask_ptr=st.len1.data_ptr(), out_f32_ptr=val_f.ptr, ldo=C, out_plane=val_p)
        return _TextFwd(te_f, te_p, te_saved, key_f, key_p, val_f, val_p)

    def _fwd_duration(self, st: _Step, tx: _TextFwd) -> _DurFwd:
        """duration predictor (efficient_tts.py:219) on V: two conv -> relu -> LayerNorm -> Dropout layers and the Linear"""
        dp, ws, rs1, C = self.m.duration_predictor, st.ws, st.rs1, self.m.n_channels
        ln0, ln1 = dp.conv[0][2], dp.conv[1][2]
        h1_f, l1_f, l1_p = ws.f32("Tdur_h1", rs1, C), ws.f32("Tdur_l1", rs1, C), ws.plane("Tdur_l1p", rs1, C, self.m.split)
        h2_f = ws.f32("Tdur_h2", rs1, C)
        dur = ws.tensor("Tdur_out", (rs1.rows,))
        w0, w1 = st.pk["dur.0"], st.pk["dur.1"]
        O.gemm(a=tx.val_p, b_ptr=w0.ptr, ldb=w0.ld, b_tap_stride=w0.tap_stride, taps=3, m=rs1.rows, n=C, act=L.ACT_RELU,
               bias=dp.conv[0][0].bias, out_f32_ptr=h1_f.ptr, ldo=C)
        O.layernorm_rows(h1_f.ptr, ln0.weight.detach(), ln0.bias.detach(), ln0.eps, st.gap1.data_ptr(), l1_f.ptr, l1_p, rs1.rows, C,
                         *st.drop.dur(0))
        O.gemm(a=l1_p, b_ptr=w1.ptr, ldb=w1.ld, b_tap_stride=w1.tap_stride, taps=3, m=rs1.rows, n=C, act=L.ACT_RELU,
               bias=dp.conv[1][0].bias, out_f32_ptr=h2_f.ptr, ldo=C)
        O.layernorm_dot(h2_f.ptr, ln1.weight.detach(), ln1.bias.detach(), ln1.eps, dp.linear.weight.detach(),
                        dp.linear.bias.detach(), st.len1.data_ptr(), 0, float(dp.offset), dur, rs1.rows, C, *st.drop.dur(1))
        return _DurFwd(h1_f, l1_f, l1_p, h2_f, dur)

    def _fwd_mel(self, st: _Step) -> _MelFwd:
        """prenet, mel encoder and, where the model has one, the query fc"""
        m, ws, rs2, C, odim, split = self.m, st.ws, st.rs2, self.m.n_channels, self.m.odim, self.m.split
        gap2 = st.gap2.data_ptr()
        mel_in_f, mel_in = ws.f32("Tmel_in_f", rs2, odim), ws.plane("Tmel_in", rs2, odim, split)
        O.pack_rows(st.speech, mel_in_f, mel_in, rs2)               # (the backward's wgrad of the prenet reads both)
        pre_f, pre_p = ws.f32("Tpre_f", rs2, C), ws.plane("Tpre_p", rs2, C, split)
        wp = st.pk["prenet"]
        pre_dp, pre_seed = st.drop.conv(LAUNCH["prenet"])            # mel_prenet's Dropout (efficient_tts.py:76-80)
        pre_z = None
        if m.act_general is not None:
            pre_z = ws.f32("Tpre_z", rs2, C)
            O.gemm(a=mel_in, b_ptr=wp.ptr, ldb=wp.ld, m=rs2.rows, n=C, bias=m.mel_prenet[0].bias, out_f32_ptr=pre_z.ptr, ldo=C)
            O.act_apply(m.act_general, pre_z.ptr, None, gap2, pre_f, pre_p, rs2.rows, C, pre_dp, pre_seed)
        elif pre_dp == 0.0 and m.fuse_prenet and odim % 8 == 0 and odim <= 128 and C % 128 == 0:
            # no Dropout on the prenet (the shipped recipe): straight from the caller's frames, whole-line stores (efts_frame_linear;
            # bit-identical to the launch below)
            O.frame_linear(x=st.speech, w=wp, bias=m.mel_prenet[0].bias, act=L.ACT_LEAKY, slope=m.slope, rs=rs2, y=pre_p, y_f32=pre_f)
        else:
            O.gemm(a=mel_in, b_ptr=wp.ptr, ldb=wp.ld, m=rs2.rows, n=C, act=L.ACT_LEAKY, slope=m.slope, bias=m.mel_prenet[0].bias,
                   rowmask_ptr=gap2, out_f32_ptr=pre_f.ptr, ldo=C, out_plane=pre_p, drop_p=pre_dp, drop_seed=pre_seed)
        if m.mel_query_fc is None:
            mh_f = mh_p = None
            q_f, q_p, me_saved = self._stack_fwd(ws, "me", "mel_encoder", st.pk, rs2, pre_f, pre_p, gap2, 2, st.drop)
        else:                                                       # efficient_tts.py:163-164: Linear(C, C) in front of the attention
            mh_f, mh_p, me_saved = self._stack_fwd(ws, "me", "mel_encoder", st.pk, rs2, pre_f, pre_p, gap2, split, st.drop)
            q_f, q_p = ws.f32("Tq_f", rs2, C), ws.plane("Tq_p", rs2, C, 2)
            wq = st.pk["qfc"]
            O.gemm(a=mh_p, b_ptr=wq.ptr, ldb=wq.ld, m=rs2.rows, n=C, bias=m.mel_query_fc.bias, rowmask_ptr=gap2,
                   out_f32_ptr=q_f.ptr, ldo=C, out_plane=q_p)
        return _MelFwd(mel_in_f, mel_in, pre_f, pre_z, (pre_dp, pre_seed), mh_f, mh_p, q_f, q_p, me_saved)

    def _fwd_alignment(self, st: _Step, mf: _MelFwd, tx: _TextFwd) -> _AlignFwd:
        """scores -> soft index -> IMV -> aligned positions e and the duration target; alpha' itself only where the expand is not fused"""
        m, ws, B, T1, T2, tl, ml, rs1, rs2 = self.m, st.ws, st.B, st.T1, st.T2, st.tl, st.ml, st.rs1, st.rs2
        scores = ws.tensor("Tscores", (B, T2, T1))
        O.gemm(a=mf.q_p, b_ptr=tx.key_p.ptr, ldb=tx.key_p.ld, m=T2, n=T1, batch=B, a_batch_stride=rs2.Tp * mf.q_p.ld,
               b_batch_stride=rs1.Tp * tx.key_p.ld, alpha=O.INV_SQRT(m.n_channels), out_f32_ptr=scores.data_ptr(), ldo=T1, out_batch_stride=T2 * T1)
        sidx, imv = ws.tensor("Tsidx", (B, T2)), ws.tensor("Timv", (B, T2))
        O.attn_soft_index(scores, T1, tl, ml, sidx, None, B, T1, T2)
        e, lde = ws.tensor("Te", (B, T1)), ws.tensor("Tlde", (B, T1))
        if m.fuse_align and O.imv_align_fits(T1, T2):
            O.imv_align(sidx, tl, ml, float(m.sigma_e), float(m.duration_offset), m.delta_e_method_1, imv, e, lde, B, T1, T2)
        else:
            O.imv_scan(sidx, tl, ml, imv, B, T2)
            O.aligned_positions(imv, tl, ml, float(m.sigma_e), float(m.duration_offset), e, lde if m.delta_e_method_1 else None, B, T1, T2)
            if not m.delta_e_method_1:                               # efficient_tts.py:205-213 (the target is detached either way)
                O.duration_target(e, tl, ml, float(m.duration_offset), False, lde, B, T1)
        ralpha = ws.tensor("Tralpha", (B, T1, T2))
        h_f, h_p = ws.f32("Texp_f", rs2, m.n_channels), ws.plane("Texp_p", rs2, m.n_channels, m.split)
        ra_p = None
        if not m._fused_expand(T1):
            ra_p = ws.plane("Tra_p", rs2, T1, 2)
            O.reconst_alpha(e, tl, ml, float(m.sigma), ralpha, ra_p, B, T1, T2, rs2.Tp)
        return _AlignFwd(scores, sidx, imv, e, lde, ralpha, ra_p, h_f, h_p)

    def _fwd_expand_decoder(self, st: _Step, al: _AlignFwd, tx: _TextFwd) -> _DecFwd:
        """H = alpha'^T V, then the decoder"""
        m, ws, B, T1, T2, rs1, rs2, C = self.m, st.ws, st.B, st.T1, st.T2, st.rs1, st.rs2, self.m.n_channels
        h_f, h_p = al.h_f, al.h_p
        if al.ra_p is None:
            # alpha' produced in registers inside the expand contraction (efts_expand); the backward packs its own operands from
            # the fp32 alpha' kept here
            O.expand(e=al.e, tl=st.tl, ml=st.ml, sigma=float(m.sigma), v=tx.val_f, rs1=rs1, rs2=rs2, alpha_out=al.ralpha, y_f32=h_f, y=h_p)
        else:
            vt = ws.raw_plane("Tvt", B * C + 136, T1, 2)
            O.pack_vt(tx.val_f, vt, B, T1, rs1.Tp, C)
            O.gemm(a=al.ra_p, b_ptr=vt.ptr, ldb=vt.ld, m=T2, n=C, batch=B, a_batch_stride=rs2.Tp * al.ra_p.ld, b_batch_stride=C * vt.ld,
                   rowmask_ptr=st.len2.data_ptr(), rowmask_batch_stride=rs2.Tp, out_f32_ptr=h_f.ptr, ldo=C, out_batch_stride=rs2.Tp * C,
                   out_plane=h_p, outb_batch_stride=rs2.Tp * h_p.ld)
        return _DecFwd(*self._stack_fwd(ws, "dec", "decoder", st.pk, rs2, h_f, h_p, st.gap2.data_ptr(), m.split, st.drop))

    def _fwd_head(self, st: _Step, dec: _DecFwd) -> F32Rows:
        m, rs2 = self.m, st.rs2
        mel = st.ws.f32("Tmel_pred", rs2, m.odim)
        wh = st.pk["head"]
        O.gemm(a=dec.d_p, b_ptr=wh.ptr, ldb=wh.ld, m=rs2.rows, n=m.odim, bias=m.mel_output_layer.bias, rowmask_ptr=st.len2.data_ptr(),
               out_f32_ptr=mel.ptr, ldo=m.odim)
        return mel

    def _fwd_losses(self, st: _Step, mel: F32Rows, du: _DurFwd, al: _AlignFwd) -> _LossFwd:
        m = self.m
        out3 = torch.empty(3, dtype=torch.float32, device=self.dev)
        # use_masking=False (fastspeech_loss.py:63-67): means over the padded tensors = the masked sums taken with full lengths
        ml_loss = st.ml if m.use_masking else torch.full_like(st.ml, st.T2)
        tl_loss = st.tl if m.use_masking else torch.full_like(st.tl, st.T1)
        O.masked_losses(mel.ptr, m.odim, st.speech, ml_loss, du.dur, al.lde, tl_loss, out3, st.ws.tensor("loss_ws", (1024,)), st.B, st.T1, st.rs1.Tp,
                        st.T2, st.rs2.Tp, m.odim)
        return _LossFwd(out3, ml_loss, tl_loss)

    def _bwd_loss(self, st: _Step, mel: F32Rows, du: _DurFwd, al: _AlignFwd, lo: _LossFwd) -> _LossBwd:
        m, ws, odim = self.m, st.ws, self.m.odim
        dmel_f = ws.f32("Bdmel_f", st.rs2, odim)
        dmel_p = ws.plane("Bdmel_p", st.rs2, odim, m.split)
        ddur = ws.tensor("Bddur", (st.rs1.rows,))
        O.loss_bwd(mel.ptr, odim, st.speech, lo.ml_loss, du.dur, al.lde, lo.tl_loss, st.gscale, dmel_f.ptr, None, ddur,
                   st.B, st.T1, st.rs1.Tp, st.T2, st.rs2.Tp, odim, split=m.split)
        return _LossBwd(dmel_f, dmel_p, ddur)

    def _bwd_duration(self, st: _Step, du: _DurFwd, tx: _TextFwd, lb: _LossBwd) -> F32Rows:
        """duration predictor (its input text_value is NOT detached: efficient_tts.py:219); returns its gradient w.r.t. V"""
        dp, ws, rs1, C, split, g = self.m.duration_predictor, st.ws, st.rs1, self.m.n_channels, self.m.split, self.g
        ln0, ln1 = dp.conv[0][2], dp.conv[1][2]

        def gname(i, k):
            return g[f"duration_predictor.conv.{i}.{k}"]
        dz2_f, dz2_p = ws.f32("Bdur_dz2", rs1, C), ws.plane("Bdur_dz2p", rs1, C, split)
        O.layernorm_bwd(du.h2_f.ptr, ln1.weight, ln1.bias, ln1.eps, None, lb.ddur, dp.linear.weight, None, dz2_f.ptr, dz2_p,
                        gname(1, "2.weight"), gname(1, "2.bias"), gname(1, "0.bias"), g["duration_predictor.linear.weight"],
                        g["duration_predictor.linear.bias"], rs1.rows, C, *st.drop.dur(1))
        dur_items = []                                           # both k3 weight gradients in one grouped launch, below
        self._wgrad_any(ws, dz2_f.ptr, dz2_p, du.l1_f.ptr, du.l1_p, C, C, 3, rs1.rows, gname(1, "0.weight"), defer=dur_items)
        G1 = ws.f32("Bdur_G1", rs1, C)
        wt = self.wt["dur.1"]
        O.gemm(a=dz2_p, b_ptr=wt.ptr, ldb=wt.ld, b_tap_stride=wt.tap_stride, taps=3, m=rs1.rows, n=C, out_f32_ptr=G1.ptr, ldo=C)
        dz1_f, dz1_p = ws.f32("Bdur_dz1", rs1, C), ws.plane("Bdur_dz1p", rs1, C, split)
        O.layernorm_bwd(du.h1_f.ptr, ln0.weight, ln0.bias, ln0.eps, G1.ptr, None, None, st.gap1.data_ptr(), dz1_f.ptr, dz1_p,
                        gname(0, "2.weight"), gname(0, "2.bias"), gname(0, "0.bias"), None, None, rs1.rows, C, *st.drop.dur(0))
        self._wgrad_any(ws, dz1_f.ptr, dz1_p, tx.val_f.ptr, tx.val_p, C, C, 3, rs1.rows, gname(0, "0.weight"), defer=dur_items)
        if dur_items:
            self._wgrad_group(ws, dur_items, C, C, rs1.rows, 3, split)
        dV_dur = ws.f32("BdV_dur", rs1, C)
        wt = self.wt["dur.0"]
        O.gemm(a=dz1_p, b_ptr=wt.ptr, ldb=wt.ld, b_tap_stride=wt.tap_stride, taps=3, m=rs1.rows, n=C, out_f32_ptr=dV_dur.ptr, ldo=C)
        return dV_dur

    def _bwd_operand_packs(self, st: _Step, tx: _TextFwd, mf: _MelFwd, al: _AlignFwd) -> _Packs:
        """operand copies of the alignment backward that depend on forward tensors only: V and alpha' as A operands, K^T, Q^T (the side
        stream idles through the decoder's backward; the main one would run them one after the other in front of their GEMMs)"""
        ws, B, T1, T2, rs1, rs2, C = st.ws, st.B, st.T1, st.T2, st.rs1, st.rs2, self.m.n_channels
        val_p2 = ws.plane("Bval_p2", rs1, C, 2)
        O.pack_rows(tx.val_f, None, val_p2, rs1, kp=C)
        ra1_p = ws.plane("Bra1_p", rs1, T2, 2)
        O.pack_rows(al.ralpha, None, ra1_p, rs1)
        kt = ws.raw_plane("Bkt", B * C + 136, T1, 2)
        O.pack_vt(tx.key_f, kt, B, T1, rs1.Tp, C)
        qt = ws.raw_plane("Bqt", B * C + 136, T2, 2)
        O.pack_vt(mf.q_f, qt, B, T2, rs2.Tp, C)
        return _Packs(val_p2, ra1_p, kt, qt)

    def _bwd_head_decoder(self, st: _Step, lb: _LossBwd, dec: _DecFwd, head_wgrad_stream, dec_wgrad_stream) -> Tuple[F32Rows, Plane]:
        """mel head (Linear 512->80, masked): bias grad + operand plane, wgrad, dgrad; then the decoder.  Returns dH, the gradient of the
        decoder's input, masked like H (efficient_tts.py:193-194), in fp32 and as a split-2 plane"""
        m, ws, rs2, C, odim, g = self.m, st.ws, st.rs2, self.m.n_channels, self.m.odim, self.g
        if m.use_masking:
            dmel_m = lb.dmel_f                                       # already zero beyond each item's length
            O.act_bwd_dropout(lb.dmel_f.ptr, None, None, None, m.slope, 0, None, lb.dmel_p, g["mel_output_layer.bias"], rs2.rows, odim)
        else:
            # the unmasked loss sees (0 - speech) on padded frames; mel_pred = masked_fill(head output) blocks that gradient (:199-200)
            dmel_m = ws.f32("Bdmel_m", rs2, odim)
            O.act_bwd_dropout(lb.dmel_f.ptr, None, None, st.len2.data_ptr(), m.slope, 0, dmel_m, lb.dmel_p, g["mel_output_layer.bias"], rs2.rows, odim)
        with self._forked(head_wgrad_stream):
            if not self._wgrad_narrow(ws, "head", lb.dmel_p, dec.d_p, odim, C, rs2.rows, g["mel_output_layer.weight"]):
                self._wgrad(ws, dmel_m.ptr, odim, dec.d_f.ptr, C, C, 1, rs2.rows, None, None, g["mel_output_layer.weight"], None)
        G = ws.f32("Bdec_Gh", rs2, C)
        wt = self.wt["head"]
        O.gemm(a=lb.dmel_p, b_ptr=wt.ptr, ldb=wt.ld, m=rs2.rows, n=C, rowmask_ptr=st.gap2.data_ptr(), out_f32_ptr=G.ptr, ldo=C)
        dH_p = ws.plane("BdH_p", rs2, C, 2)
        dH = self._stack_bwd(ws, "dec", "decoder", rs2, G, dec.dec_saved, st.gap2.data_ptr(), st.len2.data_ptr(), dH_p, wgrad_stream=dec_wgrad_stream)
        return dH, dH_p

    def _bwd_dalpha(self, st: _Step, pa: _Packs, dH_p: Plane):
        """expand backward, first half: d alpha' [B, T1, T2] = V . dH^T; also allocates the buffers of the second half (_bwd_dv), which
        may run on another stream"""
        ws, B, T1, T2, C = st.ws, st.B, st.T1, st.T2, self.m.n_channels
        dAp = ws.tensor("BdAp", (B, T1, T2))
        O.gemm(a=pa.val_p2, b_ptr=dH_p.ptr, ldb=dH_p.ld, m=T1, n=T2, batch=B, a_batch_stride=st.rs1.Tp * pa.val_p2.ld,
               b_batch_stride=st.rs2.Tp * dH_p.ld, out_f32_ptr=dAp.data_ptr(), ldo=T2, out_batch_stride=T1 * T2)
        dHt = ws.raw_plane("BdHt", B * C + 136, T2, 2)              # dH^T per item: [B][C][K = j]
        return dAp, dHt, _DV(ws.f32("BGV", st.rs1, C), ws.plane("BGV_p", st.rs1, C, self.m.split))

    def _bwd_dv(self, st: _Step, dH: F32Rows, dHt: Plane, pa: _Packs, dV_dur: F32Rows, dv: _DV) -> None:
        """expand backward, second half: dV = alpha' . dH (+ the duration predictor's dV): transpose of dH + one batched product"""
        B, T1, T2, rs1, rs2, C, (GV, GV_p) = st.B, st.T1, st.T2, st.rs1, st.rs2, self.m.n_channels, dv
        O.pack_vt(dH, dHt, B, T2, rs2.Tp, C)
        O.gemm(a=pa.ra1_p, b_ptr=dHt.ptr, ldb=dHt.ld, m=T1, n=C, batch=B, a_batch_stride=rs1.Tp * pa.ra1_p.ld, b_batch_stride=C * dHt.ld,
               resid_ptr=dV_dur.ptr, ldr=C, resid_batch_stride=rs1.Tp * C, rowmask_ptr=st.len1.data_ptr(), rowmask_batch_stride=rs1.Tp,
               out_f32_ptr=GV.ptr, ldo=C, out_batch_stride=rs1.Tp * C, out_plane=GV_p, outb_batch_stride=rs1.Tp * GV_p.ld)

    def _bwd_alignment(self, st: _Step, al: _AlignFwd, dAp: torch.Tensor, pa: _Packs) -> _AlignBwd:
        """alpha' -> e -> pi -> soft index -> scores, then dQ = scale * dS K and dS^T as the operand of dK"""
        m, ws, B, T1, T2, tl, ml, rs2, C = self.m, st.ws, st.B, st.T1, st.T2, st.tl, st.ml, st.rs2, self.m.n_channels
        de, dpi, dsx = ws.tensor("Bde", (B, T1)), ws.tensor("Bdpi", (B, T2)), ws.tensor("Bdsx", (B, T2))
        O.alpha_bwd(al.ralpha, dAp, al.e, tl, ml, float(m.sigma), ws.tensor("Br", (B, T2)), de, B, T1, T2)
        O.e_bwd(al.imv, al.e, de, tl, ml, float(m.sigma_e), ws.tensor("Bstats", (2, B, T1)), dpi, B, T1, T2)
        O.imv_bwd(al.sidx, al.imv, dpi, tl, ml, dsx, B, T2)
        dS = ws.tensor("BdS", (B, T2, T1))
        dS_p = ws.plane("BdS_p", rs2, T1, 2)
        O.attn_bwd(al.scores, T1, al.sidx, dsx, tl, ml, dS, T1, dS_p, B, T1, T2, rs2.Tp)
        GQ = ws.f32("BGQ", rs2, C)
        O.gemm(a=dS_p, b_ptr=pa.kt.ptr, ldb=pa.kt.ld, m=T2, n=C, batch=B, a_batch_stride=rs2.Tp * dS_p.ld, b_batch_stride=C * pa.kt.ld,
               alpha=O.INV_SQRT(C), out_f32_ptr=GQ.ptr, ldo=C, out_batch_stride=rs2.Tp * C)
        dSt = ws.raw_plane("BdSt", B * T1 + 264, T2, 2)             # dS^T: rows (b,i), K = j
        O.pack_vt(dS, dSt, B, T2, T2, T1)
        return _AlignBwd(de, dpi, dsx, dS, GQ, dSt)

    def _bwd_dk(self, st: _Step, ab: _AlignBwd, pa: _Packs, dv: _DV) -> Tuple[F32Rows, Plane]:
        """dK = scale * dS^T Q; with a shared key / value projection the value's gradient joins it here (residual)"""
        ws, B, T1, rs1, C = st.ws, st.B, st.T1, st.rs1, self.m.n_channels
        GK = ws.f32("BGK", rs1, C)
        GK_p = ws.plane("BGK_p", rs1, C, self.m.split)
        O.gemm(a=ab.dSt, b_ptr=pa.qt.ptr, ldb=pa.qt.ld, m=T1, n=C, batch=B, a_batch_stride=T1 * ab.dSt.ld, b_batch_stride=C * pa.qt.ld,
               alpha=O.INV_SQRT(C), resid_ptr=dv.GV.ptr if self.m.share_text_encoder_key_value else None, ldr=C, resid_batch_stride=rs1.Tp * C,
               rowmask_ptr=st.len1.data_ptr(), rowmask_batch_stride=rs1.Tp, out_f32_ptr=GK.ptr, ldo=C, out_batch_stride=rs1.Tp * C,
               out_plane=GK_p, outb_batch_stride=rs1.Tp * GK_p.ld)
        return GK, GK_p

    def _bwd_text(self, st: _Step, tx: _TextFwd, dv: _DV, GK: F32Rows, GK_p: Plane) -> F32Rows:
        """value / key Linears -> text encoder -> embedding; returns the gradient of the embedded text"""
        m, ws, rs1, C, g = self.m, st.ws, st.rs1, self.m.n_channels, self.g
        gap1 = st.gap1.data_ptr()
        shared = m.share_text_encoder_key_value                     # GK already holds dK + dV then
        sc = ws.f32("Bscratch1" + self._ws_tag, rs1, C)
        kv_items = []                                                # (value and key Linears: one grouped launch)
        if not shared:
            O.act_bwd(dv.GV.ptr, None, None, None, 0.0, 0, sc, None, g["text_encoder_value.bias"], rs1.rows, C)
            self._wgrad_any(ws, dv.GV.ptr, dv.GV_p, tx.te_f.ptr, tx.te_p, C, C, 1, rs1.rows, g["text_encoder_value.weight"], defer=kv_items)
        O.act_bwd(GK.ptr, None, None, None, 0.0, 0, sc, None, g["text_encoder_key.bias"], rs1.rows, C)
        self._wgrad_any(ws, GK.ptr, GK_p, tx.te_f.ptr, tx.te_p, C, C, 1, rs1.rows, g["text_encoder_key.weight"], defer=kv_items)
        if kv_items:
            self._wgrad_group(ws, kv_items, C, C, rs1.rows, 1, m.split)
        Gt0, Gt = ws.f32("Bte_G0", rs1, C), ws.f32("Bte_G1x", rs1, C)
        wtk = self.wt["key"]
        if shared:
            O.gemm(a=GK_p, b_ptr=wtk.ptr, ldb=wtk.ld, m=rs1.rows, n=C, rowmask_ptr=gap1, out_f32_ptr=Gt.ptr, ldo=C)
        else:
            wtv = self.wt["value"]
            O.gemm(a=dv.GV_p, b_ptr=wtv.ptr, ldb=wtv.ld, m=rs1.rows, n=C, rowmask_ptr=gap1, out_f32_ptr=Gt0.ptr, ldo=C)
            O.gemm(a=GK_p, b_ptr=wtk.ptr, ldb=wtk.ld, m=rs1.rows, n=C, resid_ptr=Gt0.ptr, ldr=C, rowmask_ptr=gap1, out_f32_ptr=Gt.ptr, ldo=C)
        Ge = self._stack_bwd(ws, "te", "text_encoder", rs1, Gt, tx.te_saved, gap1, gap1, None)
        O.embed_bwd(st.text, Ge.ptr, g["text_embedding_table.weight"], st.B, st.T1, rs1.Tp, C)
        return Ge

    def _bwd_mel_encoder(self, st: _Step, mf: _MelFwd, GQ: F32Rows, wgrad_stream) -> F32Rows:
        """query fc (where the model has one) and the mel encoder; returns the gradient of the prenet's output"""
        m, ws, rs2, C, g = self.m, st.ws, st.rs2, self.m.n_channels, self.g
        gap2 = st.gap2.data_ptr()
        G_me = GQ
        if m.mel_query_fc is not None:                               # backward of q = Linear(mel_h) (efficient_tts.py:163-164)
            GQ_p = ws.plane("BGQ_p", rs2, C, m.split)
            O.act_bwd_dropout(GQ.ptr, None, None, gap2, m.slope, 0, None, GQ_p, g["mel_query_fc.bias"], rs2.rows, C)
            self._wgrad_any(ws, GQ.ptr, GQ_p, mf.mh_f.ptr, mf.mh_p, C, C, 1, rs2.rows, g["mel_query_fc.weight"])
            G_me = ws.f32("BG_mh", rs2, C)
            wtq = self.wt["qfc"]
            O.gemm(a=GQ_p, b_ptr=wtq.ptr, ldb=wtq.ld, m=rs2.rows, n=C, rowmask_ptr=gap2, out_f32_ptr=G_me.ptr, ldo=C)
        return self._stack_bwd(ws, "me", "mel_encoder", rs2, G_me, mf.me_saved, gap2, gap2, None, wgrad_stream=wgrad_stream)

    def _bwd_prenet(self, st: _Step, mf: _MelFwd, Gm: F32Rows, wgrad_stream) -> None:
        m, ws, rs2, C, odim, g = self.m, st.ws, st.rs2, self.m.n_channels, self.m.odim, self.g
        gap2 = st.gap2.data_ptr()
        narrow = self._narrow_ok(m.split, mf.mel_in.split, C, odim, max(C, 128) * 2, mf.mel_in.ld)        # (the dZ plane allocated below is C wide)
        dzp_f = None if narrow else ws.f32("Bpre_dz", rs2, C)
        dzp_p = ws.plane("Bpre_dzp", rs2, C, m.split) if narrow else None
        if mf.pre_z is not None:
            O.act_grad(m.act_general, Gm.ptr, mf.pre_z.ptr, gap2, dzp_f, dzp_p, g["mel_prenet.0.bias"], rs2.rows, C, *mf.pre_drop)
        else:
            O.act_bwd_dropout(Gm.ptr, mf.pre_f.ptr, None, gap2, m.slope, 3, dzp_f, dzp_p, g["mel_prenet.0.bias"], rs2.rows, C, *mf.pre_drop)
        with self._forked(wgrad_stream):
            if not (narrow and self._wgrad_narrow(ws, "pre", dzp_p, mf.mel_in, C, odim, rs2.rows, g["mel_prenet.0.weight"])):
                assert dzp_f is not None
                self._wgrad(ws, dzp_f.ptr, C, mf.mel_in_f.ptr, odim, odim, 1, rs2.rows, None, None, g["mel_prenet.0.weight"], None)
