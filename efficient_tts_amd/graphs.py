"""Per-shape hipGraph cache: a plain `model(text, tl, mel, sl)` call replays its ~70 kernel launches as ONE graph launch.

The reference call site (nntts/bin/inference.py:108, nntts/trainers/efficient_tts_trainer.py:144) just calls the model; the
eager launch path of this implementation is host-bound below ~3 us per kernel, so a direct call would be ~40 % slower than
the kernels themselves.  The cache keeps that invisible: the first call of a shape runs eagerly, the second call captures
the same code path into a graph over static input copies, later calls copy the inputs in (a few us), replay and hand back
fresh clones of the outputs (the reference returns new tensors every call)."""
from __future__ import annotations

import logging
import time
from collections import OrderedDict
from typing import Callable, Sequence, Tuple

import torch


class PadTo:
    """an input of GraphCache.run that is copied into the leading corner of a zero-filled static buffer of `shape` (a ragged batch
    padded up to its bucket without a pad launch of its own)"""

    def __init__(self, t: torch.Tensor, shape):
        self.t, self.shape = t, tuple(shape)

    def padded(self) -> torch.Tensor:
        out = torch.zeros(self.shape, dtype=self.t.dtype, device=self.t.device)
        out[tuple(slice(0, n) for n in self.t.shape)].copy_(self.t)
        return out

    def into(self, static: torch.Tensor) -> None:
        static[tuple(slice(0, n) for n in self.t.shape)].copy_(self.t, non_blocking=True)


class _Entry:
    __slots__ = ("calls", "graph", "static_in", "static_out", "tag", "keepalive", "eager_only", "probe", "policy")

    def __init__(self):
        self.calls, self.graph, self.static_in, self.static_out, self.tag, self.keepalive = 0, None, None, None, None, None
        self.probe = None                # adaptive entries: (host seconds, start event, end event) of the second eager call
        self.policy = None               # ... and what they led to: "eager" | "graph" (+ the two times), for reports
        self.eager_only = False          # a capture of this shape failed once: it stays on plain launches


class GraphCache:
    EAGER_MAX_HOST_SHARE = 0.5

    def __init__(self, capacity: int = 8):
        self.capacity = capacity
        self.entries: "OrderedDict[tuple, _Entry]" = OrderedDict()
        self.captures = 0                # graphs captured so far (a replay does not count): tests read it to check which calls re-capture

    def clear(self) -> None:
        self.entries.clear()

    def run(self, key: tuple, tag, inputs: Sequence, fn: Callable[..., Tuple[torch.Tensor, ...]], keepalive=None, clone: bool = True,
            refs: Sequence[torch.Tensor] = (), adaptive: bool = False):
        """fn(*inputs, *refs) -> tuple of tensors, pure device work on the current stream (no host sync).  `tag` invalidates the
        captured graph when it changes (the buffers the launches point at were re-allocated); `keepalive` is held as long as
        the graph is (the owner of those buffers).  clone=False returns the graph's static output tensors themselves (valid until
        the next replay of this entry) instead of fresh copies.  An input may be a PadTo.  `refs`: inputs the graph reads IN PLACE
        (no static copies): buffers that are stable from call to call -- another entry's static outputs -- whose addresses join
        the tag, so a new buffer means a new capture.
        adaptive: decide per shape whether a graph pays.  A graph costs what it saves elsewhere: the inputs are copied into static
        buffers and the outputs cloned out of them on every call (8 copy launches and ~120 MB at the B = 64 teacher-forced shape:
        1.71 ms per plain call against 1.58 for the same launches issued eagerly).  The second call of a shape runs eagerly too,
        timed on the host and with events on the device; from the third call on the shape is replayed as a graph only if the host
        needed more than EAGER_MAX_HOST_SHARE of the device time to issue the launches -- i.e. unless the host runs far enough ahead
        of the device that launch latency is hidden anyway (large shapes), in which case it stays on eager launches."""
        tag = (tag, tuple(t.data_ptr() for t in refs))
        ent = self.entries.get(key)
        if ent is None:
            ent = self.entries[key] = _Entry()
            while len(self.entries) > self.capacity:
                self.entries.popitem(last=False)
        self.entries.move_to_end(key)
        if ent.graph is not None and ent.tag != tag:
            ent.graph, ent.static_in, ent.static_out, ent.keepalive, ent.calls = None, None, None, None, 1
        ent.calls += 1

        def plain():
            return fn(*[t.padded() if isinstance(t, PadTo) else t for t in inputs], *refs)

        if ent.calls == 1 or ent.eager_only:                 # first sight of this shape: plain eager run (also the warm-up)
            return plain()
        if adaptive and ent.graph is None:
            if ent.calls == 2:                               # (the first call paid the one-time costs: workspaces, plans, weight planes)
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ev0.record()
                t0 = time.perf_counter()
                out = plain()
                host = time.perf_counter() - t0
                ev1.record()
                ent.probe = (host, ev0, ev1)
                return out
            if ent.probe is not None:
                host, ev0, ev1 = ent.probe
                ev1.synchronize()
                dev_s = ev0.elapsed_time(ev1) * 1e-3
                ent.probe = None
                ent.policy = ("eager" if host <= self.EAGER_MAX_HOST_SHARE * dev_s else "graph", host, dev_s)
                if ent.policy[0] == "eager":
                    ent.eager_only = True
                    return plain()
        if ent.graph is None:
            ent.static_in = [t.padded() if isinstance(t, PadTo) else t.clone() for t in inputs]
            g = torch.cuda.CUDAGraph()
            torch.cuda.synchronize()
            try:
                # thread_local: HIP calls of OTHER threads (a DataLoader's pin-memory thread, the allocator, RCCL's proxy) during
                # the capture do not invalidate it
                with torch.cuda.graph(g, capture_error_mode="thread_local"):
                    ent.static_out = fn(*ent.static_in, *refs)
            except Exception as exc:                         # noqa: BLE001 -- any capture failure: this shape runs eagerly from now on
                logging.warning("hipGraph capture failed for %s (%s): the shape stays on eager launches", key[0], exc)
                ent.eager_only, ent.static_in, ent.static_out, ent.keepalive = True, None, None, None
                torch.cuda.synchronize()
                return plain()
            ent.graph, ent.tag, ent.keepalive = g, tag, (keepalive, tuple(refs))
            self.captures += 1
        else:
            for s, t in zip(ent.static_in, inputs):
                if isinstance(t, PadTo):
                    t.into(s)
                else:
                    s.copy_(t, non_blocking=True)
        ent.graph.replay()
        return tuple(ent.static_out) if not clone else tuple(t.clone() for t in ent.static_out)
