"""GPU (-m gpu): the training-side packers, the activation backward and the split-K sum of csrc/efts_train.hip, each alone.

    efts_pack_t  efts_pack_weight_t  efts_pack_weights_grouped  efts_act_bwd  efts_act_bwd_dropout  efts_wgrad_reduce

called directly through `efficient_tts_amd.lib` on the cases of tests/train_pack_reference.py (pinned without a device by
tests/test_train_pack_reference_cpu.py, which also asserts the condition of the bound for every reduction below).

Every output buffer is CANARY bytes before the launch, with guard bytes in front of and behind it, and is compared WHOLE: the bytes a
kernel does not own -- plane rows ch >= c, bytes past a row's K values, the gap between shifted planes, outputs of NULL-skipped items --
must still be CANARY afterwards.  Plane bytes are compared with the host encoders byte for byte (zero K padding included); dZ with the
host transcription bit for bit; sums with float64 through kernel_check._check (FACTOR, FLOOR, COND = 8, 2e-6, 2e-4, nothing widened).

efts_pack_weights_grouped: every item against a single efts_pack_weight / efts_pack_weight_t launch on it, whose plane is in turn the
host encoding of its own w_f32_out; launched with scale_ws (tile path on eligible shapes) and without (row path): identical bytes, except
the one item kind the ABI excludes without scale_ws (weight norm + dgrad plane, no folded copy), whose dgrad plane must then be NaN.

Measured on one MI355X (the worst `kernel error / e32` over the cases whose bound is the 8 * e32 branch, and the worst error where the
2e-6 floor is the bound):

    kernel                         cases  worst err / e32 (e32 > 2.5e-7)    worst err under the 2e-6 floor
    efts_pack_weight.w_f32_out        70  -                                 1.2e-07  (512x80x1 item 2)
    efts_act_bwd.dbias               124  -                                 1.7e-07  (130x128 mode=0 mask=0 split=1)
    efts_act_bwd.parts               142  -                                 2.0e-07  (130x128 mode=0 mask=0 block=0)
    efts_act_bwd.parts_sum            62  -                                 1.5e-07  (130x128 mode=0 mask=0)
    efts_act_bwd_dropout.dbias        92  -                                 1.7e-07  (65x132 mode=3 p=0.1 seed=2654435769)
    efts_wgrad_reduce.dw              14  -                                 9.6e-08  (8x64x5 nsplit=5 aligned)
    efts_wgrad_reduce.dv              14  -                                 1.3e-07  (16x80x1 nsplit=9 aligned)
    efts_wgrad_reduce.dg              14  -                                 2.1e-07  (8x64x5 nsplit=1 aligned)
    largest e32 of a case: 2.3e-07

No case has an e32 above 2.5e-7, so every sum is held to the 2e-6 floor, and the worst of them -- the atomic dbias path included -- stays
ten times below it; nothing was widened and no case is held to an a-priori bound alone.  Everything else in this file is exact: 16 pack_t,
10 pack_weight_t and 42 grouped cases byte for byte, dZ of 62 + 23 activation cases bit for bit.

Each of these one-line breaks of csrc/efts_train.hip fails here (first failing case): `taps - 1 - k` -> `k` in pack_weight_t_kernel:
test_pack_weight_t_bytes_equal_the_host_encoder[6-5-3]; `t + shift0` -> `t - shift0` in pack_t_kernel:
test_pack_t_bytes_equal_the_host_encoder[63-80-64--2-5]; the mode-5 shift `c4 & 4` dropped: test_act_bwd_vs_host[63x80-mask0-mode5]; the
`for (; sp < nsplit; ++sp)` tail of wgrad_reduce_kernel removed: test_wgrad_reduce_vs_fp64[8x64x5-nsplit1]; `rm` dropped from the dbias
accumulation: test_act_bwd_vs_host[1x4-mask1-mode0].
"""
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import gemm_reference as G
import train_pack_reference as R
from kernel_check import _call, _check, _dev, _st, load_lib

pytestmark = pytest.mark.gpu

GUARD = 256                                   # canary bytes in front of and behind every output (keeps the body 16-byte aligned)
SLOPE = R.ACT_SLOPE


@pytest.fixture(scope="module")
def lib():
    return load_lib()


class Out:
    """`nbytes` of device memory between two guards, all CANARY (or `init` in the body)"""

    def __init__(self, nbytes, init=None):
        self.n = nbytes
        self.t = torch.full((nbytes + 2 * GUARD,), G.CANARY, dtype=torch.uint8, device=_dev())
        if init is not None:
            self.t[GUARD:GUARD + nbytes] = init.contiguous().view(-1).view(torch.uint8).to(_dev())
        self.ptr = self.t.data_ptr() + GUARD

    def bytes(self):
        torch.cuda.synchronize()
        raw = self.t.cpu()
        assert bool((raw[:GUARD] == G.CANARY).all()) and bool((raw[GUARD + self.n:] == G.CANARY).all()), "write outside the buffer"
        return raw[GUARD:GUARD + self.n].clone()

    def i32(self):
        return self.bytes().view(torch.int32)

    def f32(self):
        return self.bytes().view(torch.float32)

    def untouched(self):
        return bool((self.bytes() == G.CANARY).all())


def _bits(t):
    return t.contiguous().view(-1).view(torch.int32)


def _ptr(t):
    return None if t is None else t.data_ptr()


# ---------------------------------------------------------------------------------------------------------------------
# efts_pack_t
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [1, 2])
@pytest.mark.parametrize("case", R.PACK_T_CASES, ids=lambda c: "-".join(map(str, c)))
def test_pack_t_bytes_equal_the_host_encoder(lib, case, split):
    """every shifted plane byte for byte, zero fill outside [0, rows) and up to kpad included; rows ch >= c, the row stride padding and
    the gap between the planes keep their canaries; the padding columns of a wider source row are never read"""
    rows, c, kpad, shift0, nshift, dldx, dld, dstride = case
    x = torch.randn(rows, c, generator=torch.Generator().manual_seed(rows * 1000 + c + split))
    ldx = c + dldx
    xs = torch.full((rows, ldx), 9e9)
    xs[:, :c] = x
    ld = R.kp_t(kpad, split) + dld
    stride = c * ld + dstride
    want = R.encode_t(x, rows, c, kpad, shift0, nshift, split, ld, stride)
    out = Out(want.numel())
    xd = xs.to(_dev())
    _call("efts_pack_t", lib.efts_pack_t(xd.data_ptr(), ldx, out.ptr, ld, stride, split, rows, c, shift0, nshift, kpad, _st()))
    assert torch.equal(out.bytes(), want)


# ---------------------------------------------------------------------------------------------------------------------
# efts_pack_weight_t
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [1, 2])
@pytest.mark.parametrize("cout,cin,taps", R.PACK_WEIGHT_T_CASES)
def test_pack_weight_t_bytes_equal_the_host_encoder(lib, cout, cin, taps, split):
    w = torch.randn(cout, cin, taps, generator=torch.Generator().manual_seed(cout * 7 + cin + taps * 100 + split))
    ld = G.row_bytes(cout, split) + 16
    out = Out(taps * cin * ld)
    wd = w.to(_dev())
    _call("efts_pack_weight_t", lib.efts_pack_weight_t(wd.data_ptr(), out.ptr, ld, cout, cin, taps, split, _st()))
    assert torch.equal(out.bytes().view(taps, cin, ld), R.encode_weight_t(w, split, ld, G.CANARY))


# ---------------------------------------------------------------------------------------------------------------------
# efts_pack_weights_grouped
# ---------------------------------------------------------------------------------------------------------------------
def _ldb(cout, cin, split):
    return G.row_bytes(cin, split) + 16, G.row_bytes(cout, split) + 32


@lru_cache(maxsize=2)
def _singles(lib, cout, cin, taps, split):
    """per item of R.grouped_inputs: one efts_pack_weight launch (plane + w_f32_out) and one efts_pack_weight_t launch on that w_f32_out.
    Asserted here, once: the plane is the host encoding of the launch's own w_f32_out, the dgrad plane the transposed encoding of it,
    w_f32_out the float64 fold within the bound -- bit-equal to w without a gain"""
    w, g = R.grouped_inputs(cout, cin, taps)
    ldb, ldb_t = _ldb(cout, cin, split)
    n = cout * cin * taps
    items = []
    for i, (has_g, _, _, _) in enumerate(R.GROUPED_KINDS):
        wd, gd = w[i].to(_dev()), g[i].to(_dev()) if has_g else None
        wout, plane, plane_t = Out(n * 4), Out(taps * cout * ldb), Out(taps * cin * ldb_t)
        _call("efts_pack_weight", lib.efts_pack_weight(wd.data_ptr(), _ptr(gd), wout.ptr, plane.ptr, ldb, cout, cin, taps, split, _st()))
        _call("efts_pack_weight_t", lib.efts_pack_weight_t(wout.ptr, plane_t.ptr, ldb_t, cout, cin, taps, split, _st()))
        wo = wout.f32().view(cout, cin, taps)
        pl, pt = plane.bytes().view(taps, cout, ldb), plane_t.bytes().view(taps, cin, ldb_t)
        assert torch.equal(pl, G.encode_weight(wo, split, ldb, G.CANARY))
        assert torch.equal(pt, R.encode_weight_t(wo, split, ldb_t, G.CANARY))
        if has_g:
            _check("efts_pack_weight.w_f32_out", f"{cout}x{cin}x{taps} item {i}", wo, R.fold64(w[i], g[i]), R.fold(w[i], g[i], torch.float32))
        else:
            assert torch.equal(_bits(wo), _bits(w[i]))
        items.append(SimpleNamespace(wd=wd, gd=gd, wout=wo, plane=pl, plane_t=pt))
    return items


def _grouped_launch(lib, singles, n_items, cout, cin, taps, split, with_t, scales):
    ldb, ldb_t = _ldb(cout, cin, split)
    outs, table = [], []
    for i in range(n_items):
        has_g, has_wout, has_plane, has_t = R.GROUPED_KINDS[i % len(R.GROUPED_KINDS)]
        s = singles[i]
        o = SimpleNamespace(wout=Out(cout * cin * taps * 4) if has_wout else None, plane=Out(taps * cout * ldb) if has_plane else None,
                            plane_t=Out(taps * cin * ldb_t) if has_t else None)
        outs.append(o)
        table.append([s.wd.data_ptr(), s.gd.data_ptr() if has_g else 0, o.wout.ptr if has_wout else 0, o.plane.ptr if has_plane else 0,
                      o.plane_t.ptr if has_t else 0])
    td = torch.tensor(table, dtype=torch.int64, device=_dev())
    ws = Out(n_items * cout * 4) if scales else None
    _call("efts_pack_weights_grouped", lib.efts_pack_weights_grouped(td.data_ptr(), n_items, ws.ptr if scales else None, ldb, ldb_t, cout, cin,
                                                                     taps, split, with_t, _st()))
    if scales:
        ws.bytes()                                      # (guards: the scales stay inside n_items * cout floats)
    return outs


@pytest.mark.parametrize("split", [1, 2])
@pytest.mark.parametrize("n_items", R.GROUPED_COUNTS)
@pytest.mark.parametrize("cout,cin,taps", R.GROUPED_TILE_SHAPES + R.GROUPED_ROW_SHAPES)
def test_pack_weights_grouped_items_equal_single_launches(lib, cout, cin, taps, n_items, split):
    """items with and without g, w_f32_out, plane and plane_t in one launch, with_t 0 and 1, with scale_ws (the tile path where the shape is
    eligible, else the row kernels folding from the scales) and without (the row kernels): every output equals the single launches byte
    for byte, skipped outputs keep their canaries, and the two launches agree"""
    singles = _singles(lib, cout, cin, taps, split)
    for with_t in (0, 1):
        for scales in (True, False):
            outs = _grouped_launch(lib, singles, n_items, cout, cin, taps, split, with_t, scales)
            for i, o in enumerate(outs):
                has_g, has_wout, _, _ = R.GROUPED_KINDS[i]
                s, tag = singles[i], f"item {i} with_t={with_t} scale_ws={int(scales)}"
                if o.wout is not None:
                    assert torch.equal(o.wout.i32(), _bits(s.wout)), tag
                if o.plane is not None:
                    assert torch.equal(o.plane.bytes(), s.plane.view(-1)), tag
                if o.plane_t is None:
                    continue
                if not with_t:
                    assert o.plane_t.untouched(), tag
                elif has_g and not has_wout and not scales:
                    # the excluded combination (include/efts_abi.h): nothing to fold with -- NaN, not the unfolded weight
                    pt = o.plane_t.bytes().view(taps * cin, -1)
                    hi, lo = G.decode_rows(pt, cout, split, parts=True)
                    assert bool(torch.isnan(hi[:, :cout]).all()) and (split == 1 or bool(torch.isnan(lo[:, :cout]).all())), tag
                    assert bool((hi[:, cout:] == 0).all()) and bool((pt[:, G.row_bytes(cout, split):] == G.CANARY).all()), tag
                else:
                    assert torch.equal(o.plane_t.bytes(), s.plane_t.view(-1)), tag


# ---------------------------------------------------------------------------------------------------------------------
# efts_act_bwd / efts_act_bwd_dropout
# ---------------------------------------------------------------------------------------------------------------------
def _act_device(i, mode):
    d = _dev()
    y = i.ybytes if mode in (4, 5) else i.y
    return SimpleNamespace(g=i.g.to(d), y=None if y is None else y.to(d), x=None if i.x is None else i.x.to(d),
                           rm=None if i.rm is None else i.rm.to(d))


def _act_launch(lib, dv, mode, rows, c, dz=None, plane=None, ld=0, split=1, dbias=None, drop=None):
    a = (dv.g.data_ptr(), _ptr(dv.y), _ptr(dv.x), _ptr(dv.rm), SLOPE, mode, None if dz is None else dz.ptr, None if plane is None else plane.ptr,
         ld, split, None if dbias is None else dbias.ptr, rows, c)
    if drop is None:
        _call("efts_act_bwd", lib.efts_act_bwd(*a, _st()))
    else:
        _call("efts_act_bwd_dropout", lib.efts_act_bwd_dropout(*a, drop[0], drop[1], _st()))


ACT_IDS = [f"{r}x{c}-mask{int(m)}-mode{mode}" + ("-zeros" if z else "") for r, c, m, mode, z in R.act_cases()]


@pytest.mark.parametrize("rows,c,masked,mode,zeros", R.act_cases(), ids=ACT_IDS)
def test_act_bwd_vs_host(lib, rows, c, masked, mode, zeros):
    """dZ bit for bit; the plane = the host encoding of the kernel's dZ (also written alone); dbias ADDED by the atomic path to a non-zero
    start; the per-block rows of EFTS_ACT_BWD_BIAS_PARTS per block, twice for bit equality; columns >= c, part rows >= ceil(rows / 64)
    and plane rows >= rows untouched"""
    from efficient_tts_amd import lib as L
    i, r = R.act_inputs(rows, c, mode, masked, zeros), R.act_reference(rows, c, mode, masked, zeros)
    dv = _act_device(i, mode)
    case = f"{rows}x{c} mode={mode} mask={int(masked)}" + (" zeros" if zeros else "")
    nblk = (rows + 63) // 64
    for split in (1, 2):
        ld = G.row_bytes(c, split) + 16
        dz, plane, db = Out(rows * c * 4), Out(rows * ld), Out(c * 4, i.db0)
        _act_launch(lib, dv, mode, rows, c, dz, plane, ld, split, db)
        got = dz.f32().view(rows, c)
        assert torch.equal(_bits(got), _bits(r.dz)), f"{case} split {split}"
        want_plane = G.encode_rows(got, split, ld, G.CANARY)
        assert torch.equal(plane.bytes().view(rows, ld), want_plane), f"{case} split {split}"
        _check("efts_act_bwd.dbias", f"{case} split={split}", db.f32(), i.db0.double() + r.col64, i.db0 + r.col32)
        alone = Out(rows * ld)
        _act_launch(lib, dv, mode, rows, c, None, alone, ld, split, None)
        assert torch.equal(alone.bytes().view(rows, ld), want_plane), f"{case} split {split}: plane alone"
    if zeros:
        sel = i.planted[16:48]
        neg = 0.0 if mode == 2 else np.float32(SLOPE)
        rm = torch.ones(len(sel)) if i.rm is None else i.rm[sel // c]
        if mode in (1, 2, 3):                                   # y - x == 0, y == +-0: not positive -> the slope / 0 branch
            assert torch.equal(_bits(got.view(-1)[sel]), _bits(i.g.view(-1)[sel] * (neg * rm)))
    runs = []
    for _ in range(2):
        parts, dz = Out(nblk * c * 4), Out(rows * c * 4)
        _act_launch(lib, dv, mode | L.ACT_BWD_BIAS_PARTS, rows, c, dz, None, 0, 1, parts)
        runs.append(parts.f32().view(nblk, c))
        assert torch.equal(dz.i32(), _bits(r.dz))
    assert torch.equal(_bits(runs[0]), _bits(runs[1]))
    for b in range(nblk):
        _check("efts_act_bwd.parts", f"{case} block={b}", runs[0][b], r.part64[b], r.part32[b])
    tot = [p[0].clone() for p in runs]
    for b in range(1, nblk):
        for t, p in zip(tot, runs):
            t += p[b]
    assert torch.equal(_bits(tot[0]), _bits(tot[1]))             # their fixed-order sum, run to run
    _check("efts_act_bwd.parts_sum", case, tot[0], r.col64, r.col32)


DROP_IDS = [f"{r}x{c}-mode{mode}" for r, c, mode in R.act_dropout_cases()]


@pytest.mark.parametrize("rows,c,mode", R.act_dropout_cases(), ids=DROP_IDS)
def test_act_bwd_dropout_vs_host(lib, rows, c, mode):
    """the mask regenerated from (seed, row * c + col): dZ bit for bit against keep_scale, p = 0.1 and 0.5, two seeds; the column sums of the
    masked dZ; drop_p = 0 is efts_act_bwd bit for bit"""
    i = R.act_inputs(rows, c, mode, True)
    dv = _act_device(i, mode)
    plain = Out(rows * c * 4)
    _act_launch(lib, dv, mode, rows, c, plain)
    p0 = Out(rows * c * 4)
    _act_launch(lib, dv, mode, rows, c, p0, drop=(0.0, 77))
    assert torch.equal(p0.i32(), plain.i32())
    assert torch.equal(plain.i32(), _bits(R.act_reference(rows, c, mode, True).dz))
    for drop in R.DROPS:
        r = R.act_reference(rows, c, mode, True, False, drop)
        dz, db = Out(rows * c * 4), Out(c * 4, i.db0)
        _act_launch(lib, dv, mode, rows, c, dz, dbias=db, drop=drop)
        case = f"{rows}x{c} mode={mode} p={drop[0]} seed={drop[1]}"
        assert torch.equal(dz.i32(), _bits(r.dz)), case
        _check("efts_act_bwd_dropout.dbias", case, db.f32(), i.db0.double() + r.col64, i.db0 + r.col32)


# ---------------------------------------------------------------------------------------------------------------------
# efts_wgrad_reduce
# ---------------------------------------------------------------------------------------------------------------------
WG_IDS = [f"{co}x{ci}x{t}-nsplit{s}" + ("-offset" if off else "") for co, ci, t, s, off in R.WGRAD_CASES]


@pytest.mark.parametrize("cout,cin,taps,nsplit,offset", R.WGRAD_CASES, ids=WG_IDS)
def test_wgrad_reduce_vs_fp64(lib, cout, cin, taps, nsplit, offset):
    """dW, and through the weight norm dg and dv, from a 16-byte aligned `part` (the float4 branch when cin % 4 == 0) and from a copy 4 bytes
    off (always the scalar branch): each within the bound, hence in agreement; two runs bit-equal; nothing written past the outputs"""
    part, v, g = R.wgrad_inputs(cout, cin, taps, nsplit)
    plain, chain = R.wgrad_reference(cout, cin, taps, nsplit)
    d = _dev()
    n = cout * cin * taps
    aligned = part.to(d)
    shifted = torch.zeros(part.numel() + 1, device=d)
    shifted[1:] = part.view(-1).to(d)
    vd, gd = v.to(d), g.to(d)
    assert aligned.data_ptr() % 16 == 0 and (shifted.data_ptr() + 4) % 16 == 4
    name = f"{cout}x{cin}x{taps} nsplit={nsplit}"
    order = (("offset", shifted.data_ptr() + 4), ("aligned", aligned.data_ptr())) if offset else (("aligned", aligned.data_ptr()), ("offset", shifted.data_ptr() + 4))
    for where, ptr in order:
        seen = []
        for _ in range(2):
            dw = Out(n * 4)
            _call("efts_wgrad_reduce", lib.efts_wgrad_reduce(ptr, nsplit, None, None, dw.ptr, None, cout, cin, taps, _st()))
            dv_, dg = Out(n * 4), Out(cout * 4)
            _call("efts_wgrad_reduce", lib.efts_wgrad_reduce(ptr, nsplit, vd.data_ptr(), gd.data_ptr(), dv_.ptr, dg.ptr, cout, cin, taps, _st()))
            seen.append((dw.f32(), dv_.f32(), dg.f32()))
        for a, b in zip(*seen):
            assert torch.equal(_bits(a), _bits(b)), f"{name} {where}: run to run"
        dw, dv_, dg = seen[0]
        _check("efts_wgrad_reduce.dw", f"{name} {where}", dw, *plain["dw"])
        _check("efts_wgrad_reduce.dv", f"{name} {where}", dv_, *chain["dv"])
        _check("efts_wgrad_reduce.dg", f"{name} {where}", dg, *chain["dg"])
