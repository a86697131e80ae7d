"""GPU (-m gpu): `efts_snake_aa` alone against float64  --  BigVGAN's anti-aliased Snake activation as one launch (include/efts_abi.h).

One ragged row space of 14 items with 0, 1, 2, 3, 5, 6, 7, 11, 12, 13, S - 1, S, S + 1 and 2 S + 3 units of length (S = lib.SNAKE_SEG, the rows
a lane owns: the last three items cross a segment boundary, the one before ends on it), len_mul 1 and 4, c in 4, 8, 20 (ldx = 28), 32, 132 (a
plane chunk and a half in format 1, four and a bit in formats 2 / 3), a = exp(0.5 randn), inv_b likewise, x = 2 randn.  Every row of x
that the definition does not read (past a length, between items, the guard rows) holds NaN.

Bound: `kernel_check._check`, max(8 e32, 2e-6) of max |ref| with 8 e32 <= 2e-4 asserted, e32 the error of tests/bigvgan_reference.py's torch-op
composition in float32 on the CPU; plus the resolution of the plane format (2^-8, 2^-16, 0), as the x_plane / mean_act rows of
tests/test_vocoder_stages_gpu.py.  With ==: rows past a length are 0; gap rows, guard rows and columns past c keep their prefill (7.0 / 0xAB);
the plane's padding columns are 0; every item equals the same item run alone at row 0; a captured call replays the eager bits.
The worst error per format and its yardstick go to profiles/snake_aa_error.json.
"""
import ctypes
import functools
import json
import os

import pytest
import torch

import bigvgan_reference as BR
from kernel_check import FACTOR, FLOOR, _check, _dev, _rel, _st, load_lib, unpack_plane

pytestmark = pytest.mark.gpu

RESOLUTION = {None: 0.0, 3: 0.0, 2: 2.0 ** -16, 1: 2.0 ** -8}
GUARD = 3
WORST = {}


def _lens():
    from efficient_tts_amd import lib as L
    S = L.SNAKE_SEG
    return [0, 1, 2, 3, 5, 6, 7, 11, 12, 13, S - 1, S, S + 1, 2 * S + 3]


@pytest.fixture(scope="module")
def lib():
    lib = load_lib()
    yield lib
    if WORST:
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "snake_aa_error.json")
        with open(path, "w") as f:
            json.dump({"kernel": "efts_snake_aa", "metric": "max |got - ref64| / max |ref64| over the 14 items of a case",
                       "yardstick": "max(8 * e32, 2e-6) + resolution of the format; e32: the float32 torch-op composition on the CPU",
                       "worst": WORST}, f, indent=1, sort_keys=True)
            f.write("\n")


@functools.lru_cache(maxsize=None)
def _case(c, len_mul):
    """x [B][rows][c] float32 (live rows only), a, inv_b and the two references per item"""
    g = torch.Generator().manual_seed(100 * c + len_mul)
    a, inv_b = torch.exp(0.5 * torch.randn(c, generator=g)), torch.exp(0.5 * torch.randn(c, generator=g))
    xs, r64, r32 = [], [], []
    for n in _lens():
        x = 2 * torch.randn(n * len_mul, c, generator=g)
        xs.append(x)
        if n:
            xt = x.t().contiguous()[None]
            r64.append(BR.activation1d(xt.double(), a, inv_b)[0].t())
            r32.append(BR.activation1d(xt, a, inv_b)[0].t())
        else:
            r64.append(torch.zeros(0, c, dtype=torch.float64))
            r32.append(torch.zeros(0, c))
    return a, inv_b, xs, r64, r32


def _launch(lib, x, ldx, lens, a, inv_b, B, pitch, T, len_mul, c, out=None, ldo=0, plane=None, ldp=0, split=0, row0=GUARD):
    from efficient_tts_amd import lib as L
    g = L.SnakeAAArgs()
    g.x, g.ldx, g.lengths, g.a, g.inv_b = x.data_ptr() + row0 * ldx * 4, ldx, lens.data_ptr(), a.data_ptr(), inv_b.data_ptr()
    if out is not None:
        g.out, g.ldo = out.data_ptr() + row0 * ldo * 4, ldo
    if plane is not None:
        g.plane, g.ld_plane, g.split = plane.data_ptr() + row0 * ldp, ldp, split
    g.B, g.pitch, g.T, g.len_mul, g.c = B, pitch, T, len_mul, c
    return lib.efts_snake_aa(ctypes.byref(g), _st())


def _nchunk(c, split):
    k = 64 if split == 1 else 32
    return (c + k - 1) // k


@pytest.mark.parametrize("len_mul", [1, 4])
@pytest.mark.parametrize("c", [4, 8, 20, 32, 132])
def test_snake_aa_vs_fp64(lib, c, len_mul):
    from efficient_tts_amd import lib as L
    dev = _dev()
    a, inv_b, xs, r64, r32 = _case(c, len_mul)
    lens, B = _lens(), len(_lens())
    T = max(lens)
    rows_item, pitch = T * len_mul, T * len_mul + 6
    ldx = 28 if c == 20 else c
    alloc = GUARD + B * pitch + GUARD
    x = torch.full((alloc, ldx), float("nan"))
    for b, xb in enumerate(xs):
        x[GUARD + b * pitch:GUARD + b * pitch + xb.shape[0], :c] = xb
    x_d, a_d, ib_d = x.to(dev), a.to(dev), inv_b.to(dev)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    ref64, ref32 = torch.cat(r64), torch.cat(r32)
    live = torch.zeros(alloc, dtype=torch.bool)           # rows of items below their length
    written = torch.zeros(alloc, dtype=torch.bool)        # rows the launch writes
    for b, n in enumerate(lens):
        live[GUARD + b * pitch:GUARD + b * pitch + n * len_mul] = True
        written[GUARD + b * pitch:GUARD + b * pitch + rows_item] = True

    def buffers(split, with_out):
        ldo = c + 4
        out = torch.full((alloc, ldo), 7.0, device=dev) if with_out else None
        ldp = 0 if split is None else _nchunk(c, split) * 128 + (128 if c == 8 else 0)
        pl = torch.full((alloc, ldp), 0xAB, dtype=torch.uint8, device=dev) if split else None
        return out, ldo, pl, ldp

    def alone(b, split, with_out):
        """item b as a batch of one at row 0 of buffers of its own: (fp32 rows, plane rows) of its rows_item rows"""
        n = lens[b] * len_mul
        xa = torch.full((GUARD + rows_item + GUARD, ldx), float("nan"))
        xa[GUARD:GUARD + n, :c] = xs[b]
        out, ldo, pl, ldp = buffers(split, with_out)
        rc = _launch(lib, xa.to(dev), ldx, lens_d[b:b + 1].clone(), a_d, ib_d, 1, rows_item, T, len_mul, c, out, ldo, pl, ldp, split or 0)
        L.check(rc, "efts_snake_aa")
        return (None if out is None else out[GUARD:GUARD + rows_item, :c], None if pl is None else pl[GUARD:GUARD + rows_item])

    for split, with_out in ((None, True), (1, False), (2, True), (3, False)):
        out, ldo, pl, ldp = buffers(split, with_out)
        L.check(_launch(lib, x_d, ldx, lens_d, a_d, ib_d, B, pitch, T, len_mul, c, out, ldo, pl, ldp, split or 0), "efts_snake_aa")
        torch.cuda.synchronize()
        case = f"c={c} len_mul={len_mul} ldx={ldx} out={with_out} plane={split}"
        eager = (None if out is None else out.clone(), None if pl is None else pl.clone())
        if out is not None:
            o = out.cpu()
            _check("efts_snake_aa.fp32", case, o[live][:, :c], ref64, ref32)
            _note("fp32", case, o[live][:, :c], ref64, ref32, 0.0)
            assert bool((o[written & ~live][:, :c] == 0).all()), "rows past a length must be 0"
            assert bool((o[~written] == 7.0).all()) and bool((o[:, c:] == 7.0).all()), "gap rows, guard rows, columns past c: untouched"
        if pl is not None:
            raw = pl.cpu()
            nb = _nchunk(c, split) * 128
            assert bool((raw[~written] == 0xAB).all()) and bool((raw[:, nb:] == 0xAB).all()), "gap rows, guard rows, bytes past the chunks: untouched"
            kp = _nchunk(c, split) * (64 if split == 1 else 32)
            val = unpack_plane(raw[:, :nb].contiguous(), 1, alloc, alloc, kp, split)[0]
            assert bool((val[written][:, c:] == 0).all()), "the plane's padding columns must be 0"
            assert bool((val[written & ~live] == 0).all()), "rows past a length must be 0"
            _check(f"efts_snake_aa.plane{split}", case, val[live][:, :c], ref64, ref32, extra=RESOLUTION[split])
            _note(f"plane{split}", case, val[live][:, :c], ref64, ref32, RESOLUTION[split])
        # every item alone at row 0: the same bits
        for b in range(B):
            o1, p1 = alone(b, split, with_out)
            lo = GUARD + b * pitch
            if out is not None:
                assert torch.equal(out[lo:lo + rows_item, :c].contiguous().view(torch.int32), o1.contiguous().view(torch.int32)), (case, b)
            if pl is not None:
                assert torch.equal(pl[lo:lo + rows_item], p1), (case, b)
        # a captured call replays the eager bits
        out2, _, pl2, _ = buffers(split, with_out)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                L.check(_launch(lib, x_d, ldx, lens_d, a_d, ib_d, B, pitch, T, len_mul, c, out2, ldo, pl2, ldp, split or 0), "efts_snake_aa")
        torch.cuda.current_stream().wait_stream(side)
        for buf, fill in ((out2, 7.0), (pl2, 0xAB)):
            if buf is not None:
                buf.fill_(fill)
        graph.replay()
        torch.cuda.synchronize()
        if out is not None:
            assert torch.equal(out2.view(torch.int32), eager[0].view(torch.int32)), case
        if pl is not None:
            assert torch.equal(pl2, eager[1]), case


def _note(fmt, case, got, ref64, ref32, res):
    err, e32 = _rel(got.double(), ref64), _rel(ref32.double(), ref64)
    bound = max(FACTOR * e32, FLOOR) + res
    if fmt not in WORST or err / bound > WORST[fmt]["err"] / WORST[fmt]["bound"]:
        WORST[fmt] = dict(case=case, err=err, e32=e32, bound=bound)


def test_snake_aa_refuses_bad_arguments(lib):
    dev = _dev()
    x = torch.zeros(GUARD + 16 + GUARD, 8, device=dev)
    a = torch.ones(8, device=dev)
    lens = torch.tensor([4], dtype=torch.int32, device=dev)
    out = torch.zeros_like(x)

    def rc(**kw):
        args = dict(x=x, ldx=8, lens=lens, a=a, inv_b=a, B=1, pitch=16, T=4, len_mul=1, c=8, out=out, ldo=8)
        args.update(kw)
        return _launch(lib, args["x"], args["ldx"], args["lens"], args["a"], args["inv_b"], args["B"], args["pitch"], args["T"], args["len_mul"],
                       args["c"], args["out"], args["ldo"], args.get("plane"), args.get("ldp", 0), args.get("split", 0), row0=args.get("row0", 0))
    assert rc() == 0
    assert rc(c=6) == -2 and b"multiple of 4" in lib.efts_last_error()                       # EFTS_ESHAPE
    assert rc(c=0) == -2 and rc(T=17) == -2 and rc(B=0) == -2 and rc(ldx=4) == -2
    assert rc(out=None) == -1 and b"neither" in lib.efts_last_error()                          # EFTS_EINVAL: no output at all
    assert rc(out=None, plane=torch.zeros(22, 128, dtype=torch.uint8, device=dev), ldp=128, split=4) == -1
    from efficient_tts_amd import lib as L
    g = L.SnakeAAArgs()
    assert lib.efts_snake_aa(ctypes.byref(g), _st()) == -1 and b"null operand" in lib.efts_last_error()
    assert lib.efts_snake_aa(None, _st()) == -1
    assert rc(x=x.view(-1)[1:]) == -3 and b"aligned" in lib.efts_last_error()                 # EFTS_EALIGN: x 4 bytes off
    assert rc(a=torch.ones(9, device=dev)[1:]) == -3 and rc(ldo=10) == -3
    torch.cuda.synchronize()
