"""The B operand planes every launch reads EfficientTTSCNN's Conv1d / Linear weights from, and the one place that decides when they are
repacked (weight-norm fold fused; equally shaped weights share one `efts_pack_weights_grouped` launch through a device-side item table).
Eval paths call `get()`; the training pass calls `schedule()`, then `issue(phase)` for every phase.  A repack counts as done once its
last phase has been issued: until then, and after any failure on the way, the planes are stale and the next call repacks.  Whoever
changes the parameters in place without a version bump (the fused optimizer, a broadcast, a captured step) calls `invalidate()`."""
from __future__ import annotations

from typing import Callable, Dict, Optional

import torch

from . import lib as L
from . import ops as O
from .ops import PackedWeight, Plane, Rows


class WeightPlanes:
    # Every method that reads the parameters takes the model: a reference kept here would make each model a reference cycle, which only
    # the cyclic garbage collector frees -- at any allocation, also inside a graph capture, where freeing the model's graphs aborts
    def __init__(self):
        self.packed: Dict[str, PackedWeight] = {}
        self.sig = None                 # (data_ptr, _version) of every parameter the planes hold; None: stale
        self.ptr_sig = 0                # parameter storage identity at the last repack (captured graphs hold these pointers)
        self.gen = 0                    # completed repacks: what caches derived from the planes compare
        self.derived = False            # the last repack also wrote the training engine's folded fp32 weights and dgrad planes
        self.tables: Dict[tuple, tuple] = {}
        # the repack in progress: phase -> its launches not issued yet, all of its phases, the (sig, derived) its last phase commits
        self.pending: Dict[Optional[str], list] = {}
        self.phases, self.done = (), None
        # tap table of text-encoder layer 0: geometry, table, staging plane, symbol ids, the repack it was built from
        self.te0_geo = self.te0_tab = self.te0_plane = self.te0_ids = self.te0_gen = None

    def invalidate(self) -> None:
        """the next get() / schedule() repacks (and a repack in progress does not count)"""
        self.sig = self.done = None

    def tag(self) -> tuple:
        """the weight part of a captured graph's tag: parameter storages, plane and tap-table addresses"""
        return self.ptr_sig, tuple(w.ptr for w in self.packed.values()), 0 if self.te0_tab is None else self.te0_tab.data_ptr()

    @staticmethod
    def modules(m):
        """(name, module, cout, cin, taps) of every packed weight of model `m`"""
        mods = [(f"{blk}.{i}", layer.conv[0]) for blk in ("text_encoder", "mel_encoder", "decoder") for i, layer in enumerate(getattr(m, blk).layers)]
        mods += [(f"dur.{i}", seq[0]) for i, seq in enumerate(m.duration_predictor.conv)]
        mods += [("key", m.text_encoder_key), ("prenet", m.mel_prenet[0]), ("head", m.mel_output_layer)]
        if not m.share_text_encoder_key_value:
            mods.append(("value", m.text_encoder_value))
        if m.mel_query_fc is not None:
            mods.append(("qfc", m.mel_query_fc))
        return [(name, mod, *(mod.weight_v if hasattr(mod, "weight_g") else mod.weight).shape[:2], getattr(mod, "kernel_size", (1,))[0])
                for name, mod in mods]

    def _signature(self, m, params) -> tuple:
        if self.pending:
            raise RuntimeError(f"weight repack phases {sorted(self.pending, key=str)} were scheduled but never issued")
        return tuple((p.data_ptr(), p._version) for p in (params if params is not None else m.parameters()))

    def get(self, m, params=None) -> Dict[str, PackedWeight]:
        """the planes of model `m`, repacked first (on the current stream) if a parameter changed"""
        sig = self._signature(m, params)
        if sig != self.sig:
            self._schedule(m, sig, {}, {}, lambda name: None)
            self.issue(None)
        return self.packed

    def schedule(self, m, folded, wt: Dict[str, PackedWeight], params, phase_of: Callable[[str], str]) -> Dict[str, PackedWeight]:
        """the training pass's repack, which also writes `folded[name]` (fp32 [cout][cin][taps]: g * v / ||v|| of a weight-normed conv)
        and `wt[name]` (the transposed + tap-flipped dgrad plane) -- also when the parameters are unchanged but the last repack (an eval
        forward) did not.  Launches nothing: issue(phase) enqueues those of the weights with phase_of(name) == phase."""
        sig = self._signature(m, params)
        if sig != self.sig or not self.derived:
            self._schedule(m, sig, folded, wt, phase_of)
        return self.packed

    def issue(self, phase: Optional[str]) -> None:
        """enqueue the launches of `phase` of the scheduled repack on the current stream (none if nothing needed repacking)"""
        try:
            if phase not in self.phases:
                raise ValueError(f"no weight repack phase {phase!r} (phases: {self.phases})")
            for args in self.pending.pop(phase, ()):
                L.check(L.load().efts_pack_weights_grouped(*args, O._stream()), "efts_pack_weights_grouped")
        except BaseException:
            self.pending, self.done = {}, None          # the repack is abandoned: the planes stay stale
            raise
        if not self.pending and self.done is not None:
            (self.sig, self.derived), self.done = self.done, None
            self.ptr_sig, self.gen = hash(tuple(a for a, _ in self.sig)), self.gen + 1

    def _schedule(self, m, sig, folded, wt, phase_of) -> None:
        pk = self.packed
        self.sig = None                                  # stale from here until the last phase is issued
        dev = m.text_embedding_table.weight.device
        groups: Dict[tuple, list] = {}
        for name, mod, cout, cin, taps in self.modules(m):
            if name not in pk or pk[name].buf.device != dev:
                pk[name] = PackedWeight(cout, cin, taps, m.split, dev)
            groups.setdefault((cout, cin, taps, name in wt, phase_of(name)), []).append((name, mod))
        table_rows, launches = [], []
        for (cout, cin, taps, with_t, phase), members in groups.items():
            first = len(table_rows)
            fold = cout % 64 or cin % 64 or taps > 5          # not the library's one-pass path: the row pack kernels read a folded copy
            for name, mod in members:
                wn = hasattr(mod, "weight_g")
                fo = folded.get(name) if wn and fold else None
                if wn and fold and with_t and fo is None:
                    raise L.EftsError(f"{name}: the row pack kernels need a folded fp32 copy for the dgrad plane")
                w = (mod.weight_v if wn else mod.weight).detach()
                assert w.is_contiguous()
                table_rows.append((w.data_ptr(), mod.weight_g.data_ptr() if wn else 0, 0 if fo is None else fo.data_ptr(), pk[name].ptr,
                                   wt[name].ptr if with_t else 0))
            launches.append((first, len(members), pk[members[0][0]].ld, wt[members[0][0]].ld if with_t else 0, cout, cin, taps,
                             int(with_t), phase))
        key, tables = tuple(table_rows), self.tables
        if key not in tables:
            # Built once per item list and KEPT: the eval forward and the training engine alternate between two lists (with and without
            # the dgrad planes), and a training step captured as a hipGraph keeps launching with the table it was captured with (a
            # replaced table would be freed memory under that graph).  Least recently used ones go beyond 8: those belong to parameter
            # storages that no longer exist, which a captured step can no longer be replayed with either (its tag holds the storages)
            while len(tables) >= 8:
                tables.pop(next(iter(tables)))
            # (scale workspace: one region per phase -- the launches of a phase run in order on one stream, different phases may overlap)
            phases = sorted({t[8] for t in launches}, key=str)
            region = max(n * co for _, n, _, _, co, _, _, _, _ in launches)
            tables[key] = (torch.tensor(table_rows, dtype=torch.int64, device=dev), torch.empty(len(phases) * region, device=dev),
                           {ph: i * region * 4 for i, ph in enumerate(phases)})
        table, scale, region_of = tables[key] = tables.pop(key)         # (most recently used last)
        for first, n, ld, ld_t, cout, cin, taps, with_t, phase in launches:
            self.pending.setdefault(phase, []).append((table.data_ptr() + first * 40, n, scale.data_ptr() + region_of[phase], ld, ld_t,
                                                       cout, cin, taps, m.split, with_t))
        self.phases, self.done = tuple(self.pending), (sig, bool(wt))

    def te0_table(self, m) -> torch.Tensor:
        """tap_table [k_size][num_symbols][C] of text-encoder layer 0 from the current planes: tap k's weights applied to every symbol's
        embedding in the model's operand format (k_size one-tap efts_gemm launches).  ONE table (and staging plane) per (device, geometry),
        rebuilt IN PLACE after every repack: captured graphs bake the table's address into their efts_embed_conv launch, so a fresh
        allocation per repack would leave them reading a freed or stale table; the stream orders the rebuild before a replay"""
        if self.te0_gen == self.gen:
            return self.te0_tab
        table = m.text_embedding_table.weight.detach()
        V, C, K, dev = table.shape[0], m.n_channels, m.k_size, table.device
        rsv = Rows(1, V)
        if self.te0_geo != (dev, K, V, C, m.split):
            self.te0_geo = (dev, K, V, C, m.split)
            self.te0_tab = torch.empty(K, V, C, dtype=torch.float32, device=dev)
            self.te0_plane = Plane.for_rows(rsv, C, m.split, dev)
            self.te0_ids = torch.arange(V, device=dev)[None]
        with O.stream_scope():
            O.embed(self.te0_ids, table, None, self.te0_plane, rsv)
            w = self.packed["text_encoder.0"]
            for k in range(K):
                O.gemm(a=self.te0_plane, b_ptr=w.ptr + k * w.tap_stride, ldb=w.ld, m=V, n=C, out_f32_ptr=self.te0_tab[k].data_ptr(), ldo=C,
                       tiling=L.TILING_GENERIC)
        self.te0_gen = self.gen
        return self.te0_tab
