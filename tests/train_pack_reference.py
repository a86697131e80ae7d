"""The training-side packers, the activation backward and the split-K sum of csrc/efts_train.hip on the host  --  TEST INFRASTRUCTURE for
tests/test_train_pack_reference_cpu.py (no device) and tests/test_train_pack_kernels_gpu.py.  Plain module: importing it needs neither a
GPU nor the library.

What is here:
  * encode_t / encode_weight_t: the planes of efts_pack_t and efts_pack_weight_t, built on gemm_reference.encode_rows;
  * fold: the weight-norm fold g v / ||v|| in float64 (fold64) and float32;
  * keep_scale: hash_u32 / drop_scale of csrc/efts_internal.h in numpy uint32, with the launch's thresh and inv_keep;
  * sign_words / sign_bits: the mode-4 and mode-5 sign inputs of efts_act_bwd from a boolean tensor;
  * act_bwd_ref: dZ in float32 with the kernel's multiplication order, its column sums in float64 and float32, per 64-row block too;
  * wgrad_reduce_ref: dW, and with weight norm dg and dv, each as a float64 / float32 pair;
  * the case tables and the deterministic inputs both test files share.
"""
import zlib
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import torch

from gemm_reference import CANARY, encode_rows, row_bytes

# ------------------------------------------------------------------------------------------------------------ the cases
# efts_pack_t: (rows, c, kpad, shift0, nshift, ldx - c, ld_plane - minimum, plane_stride - c * ld_plane)
PACK_T_CASES = (
    (1, 4, 64, 0, 1, 0, 0, 0),
    (63, 80, 64, -2, 5, 0, 0, 0),
    (65, 33, 128, -1, 3, 0, 0, 0),              # the channel count is not a multiple of 32
    (130, 512, 192, -5, 11, 0, 0, 0),           # the widest stage the kernel allows
    (70, 80, 256, 0, 1, 0, 0, 0),               # whole 64-row blocks beyond `rows`: zero, not stale
    (64, 32, 64, 3, 2, 0, 0, 0),                # a positive shift
    (63, 36, 64, -1, 3, 5, 48, 0),              # a padded source row stride and ld_plane above the minimum
    (65, 40, 128, -1, 3, 0, 0, 272),            # a gap between the shifted planes
)
PACK_WEIGHT_T_CASES = ((6, 5, 3), (130, 7, 5), (80, 512, 1), (512, 80, 1), (64, 64, 5))         # (cout, cin, taps); 6: cout % 4 != 0
GROUPED_TILE_SHAPES = ((64, 64, 5), (128, 192, 3), (512, 512, 5))
GROUPED_ROW_SHAPES = ((80, 512, 1), (512, 80, 1), (64, 64, 7), (6, 5, 3))
GROUPED_COUNTS = (1, 3, 8)
# (g, w_f32_out, plane, plane_t) of item i % 8 of a grouped launch.  Kind 2 -- weight norm and a dgrad plane but no folded copy -- is the one
# the row kernels can only serve from the scales in scale_ws (include/efts_abi.h at efts_pack_weights_grouped)
GROUPED_KINDS = (
    (True, True, True, True),
    (False, False, True, True),
    (True, False, True, True),
    (False, True, True, False),
    (True, True, False, True),
    (True, False, True, False),
    (False, True, False, True),
    (True, False, False, True),
)
ACT_SHAPES = ((1, 4), (63, 80), (65, 132), (130, 128), (200, 512))
ACT_ZERO_SHAPE = (65, 128)                      # the planted-zero case: every mode accepts it
ACT_MODES = (0, 1, 2, 3, 4, 5)
ACT_SLOPE = 0.1
DROP_PS, DROP_SEEDS = (0.1, 0.5), (77, 0x9E3779B9)
WGRAD_CASES = (                                 # (cout, cin, taps, nsplit, primary run on a `part` 4 bytes off its alignment)
    (8, 64, 5, 1, False),
    (8, 64, 5, 4, False),
    (8, 64, 5, 5, False),
    (16, 80, 1, 9, False),
    (5, 7, 3, 3, False),                        # cin % 4 != 0: the scalar branch
    (8, 64, 3, 6, True),                        # a misaligned pointer: the scalar branch
    (512, 512, 5, 3, False),
)


def act_mode_runs(mode, c):
    """does efts_act_bwd accept `mode` at `c` columns?  (c % 4 == 0 throughout)"""
    return c % 128 == 0 if mode == 4 else c % 8 == 0 if mode == 5 else True


DROPS = tuple((p, seed) for p in DROP_PS for seed in DROP_SEEDS)


def act_cases():
    """(rows, c, masked, mode, zeros) of every efts_act_bwd case"""
    return [(rows, c, masked, mode, (rows, c) == ACT_ZERO_SHAPE) for rows, c in ACT_SHAPES + (ACT_ZERO_SHAPE,) for masked in (False, True)
            for mode in ACT_MODES if act_mode_runs(mode, c)]


def act_dropout_cases():
    """(rows, c, mode): modes 0 to 3 on every shape, 5 where c % 8 == 0; all with a row mask"""
    return [(rows, c, mode) for rows, c in ACT_SHAPES for mode in (0, 1, 2, 3, 5) if act_mode_runs(mode, c)]


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


# ------------------------------------------------------------------------------------------------------------ packers
def kp_t(kpad, split):
    """efts_pack_t rows hold exactly kpad values (kpad % 64 == 0 is a multiple of both chunk sizes)"""
    assert kpad % 64 == 0
    return row_bytes(kpad, split)


def encode_t(x, rows, c, kpad, shift0, nshift, split, ld, plane_stride):
    """the bytes of efts_pack_t's output: uint8 [(nshift - 1) * plane_stride + c * ld].  Plane s (at s * plane_stride), row ch (stride ld) is
    the encoding of [x[t + shift0 + s][ch] for t < kpad], 0 where t + shift0 + s lies outside [0, rows); every other byte is CANARY"""
    x = x.detach().float()
    assert x.shape == (rows, c) and ld >= kp_t(kpad, split) and plane_stride >= c * ld
    out = torch.full(((nshift - 1) * plane_stride + c * ld,), CANARY, dtype=torch.uint8)
    t = torch.arange(kpad)
    for s in range(nshift):
        src = t + shift0 + s
        ok = (src >= 0) & (src < rows)
        xt = torch.zeros(c, kpad)
        xt[:, ok] = x[src[ok]].T
        out[s * plane_stride:s * plane_stride + c * ld] = encode_rows(xt, split, ld, CANARY).reshape(-1)
    return out


def encode_weight_t(w, split, ld=None, fill=0):
    """w fp32 [cout][cin][taps] -> dgrad plane [taps][cin][ld]: plane[taps - 1 - k][ci] = encode(w[:, ci, k]), K = cout"""
    cout, cin, taps = w.shape
    rows = torch.stack([w[:, :, taps - 1 - j].T for j in range(taps)]).reshape(taps * cin, cout)
    return encode_rows(rows, split, ld, fill).view(taps, cin, -1)


def fold(v, g, dtype):
    """the weight-norm fold g v / ||v|| (norm over cin * taps) in `dtype`"""
    v, g = v.to(dtype), g.to(dtype)
    return g[:, None, None] * v / v.pow(2).sum((1, 2), keepdim=True).sqrt()


def fold64(v, g):
    return fold(v, g, torch.float64)


@lru_cache(maxsize=2)
def grouped_inputs(cout, cin, taps):
    """weights and gains of the 8 items of a grouped launch (a launch of n items takes the first n)"""
    gen = _gen("grouped", cout, cin, taps)
    w = torch.randn(len(GROUPED_KINDS), cout, cin, taps, generator=gen) / (cin * taps) ** 0.5
    g = torch.rand(len(GROUPED_KINDS), cout, generator=gen) + 0.5
    return w, g


# ------------------------------------------------------------------------------------------------------------ dropout
def hash_u32(x):
    """hash_u32 of csrc/efts_internal.h on a numpy array, in uint32 arithmetic"""
    x = np.asarray(x).astype(np.uint32)
    with np.errstate(over="ignore"):
        x = x ^ (x >> np.uint32(16))
        x = x * np.uint32(0x7FEB352D)
        x = x ^ (x >> np.uint32(15))
        x = x * np.uint32(0x846CA68B)
        x = x ^ (x >> np.uint32(16))
    return x


def drop_params(p):
    """(thresh, inv_keep) as efts_act_bwd_dropout computes them from its float argument: uint32(p * 2^32), float32(1 / (1 - p))"""
    p32 = np.float32(p)
    thresh = np.uint32(int(float(p32) * 4294967296.0))
    inv_keep = np.float32(1.0) / (np.float32(1.0) - p32)
    return thresh, inv_keep


def keep_scale(seed, idx, p):
    """drop_scale(hash_u32(seed), idx, thresh, inv_keep): float32 array, inv_keep where the element is kept and 0 where it is dropped"""
    thresh, inv_keep = drop_params(p)
    seed_h = hash_u32(np.uint32(seed & 0xFFFFFFFF))
    h = hash_u32(np.asarray(idx).astype(np.uint32) ^ seed_h)
    return np.where(h >= thresh, inv_keep, np.float32(0.0)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------ activation backward
def sign_words(pos):
    """bool [rows][c], c % 128 == 0 -> the mode-4 bytes uint8 [rows][c / 8]: 16 bytes per row and 128-column group, word u, bit q = column
    4 q + u of the group (efts_gemm's `sign_mask`)"""
    rows, c = pos.shape
    assert c % 128 == 0
    p = pos.numpy().astype(np.uint32).reshape(rows, c // 128, 32, 4)                  # [row][group][q][u]
    words = (p << np.arange(32, dtype=np.uint32)[None, None, :, None]).sum(2, dtype=np.uint32)      # [row][group][u]
    return torch.from_numpy(np.ascontiguousarray(words).astype("<u4").view(np.uint8).reshape(rows, c // 8).copy())


def sign_bits(pos):
    """bool [rows][c], c % 8 == 0 -> the mode-5 bytes uint8 [rows][c / 8]: bit j of byte cc = column 8 cc + j (efts_resconv5's `sign_bits`)"""
    rows, c = pos.shape
    assert c % 8 == 0
    return torch.from_numpy(np.packbits(pos.numpy().astype(np.uint8), axis=1, bitorder="little").copy())


def act_bwd_ref(g, y, x, rowmask, slope, mode, drop=None):
    """efts_act_bwd / efts_act_bwd_dropout on the host.  g, y, x: float32 [rows][c] (y: the bool tensor the sign words / bits were built
    from for modes 4 and 5; unused inputs None); rowmask float32 [rows] or None; drop: None or (p, seed).
    -> dz       float32, the kernel's multiplication order g * ((m * keep) * rm): bit-exact
       col64/32 column sums of dZ in float64 (of the float64 products) and in float32
       part64/32 the same per 64-row block, [ceil(rows / 64)][c]"""
    rows, c = g.shape
    sl = torch.tensor(slope, dtype=torch.float32)
    one = torch.ones((), dtype=torch.float32)
    if mode == 0:
        m = torch.ones(rows, c)
    elif mode == 1:
        m = torch.where((y - x) > 0, one, sl)
    elif mode == 2:
        m = torch.where(y > 0, one, torch.zeros(()))
    elif mode == 3:
        m = torch.where(y > 0, one, sl)
    elif mode in (4, 5):
        assert y.dtype == torch.bool
        m = torch.where(y, one, sl)
    else:
        raise ValueError(mode)
    keep = torch.ones(rows, c)
    if drop is not None:
        p, seed = drop
        keep = torch.from_numpy(keep_scale(seed, np.arange(rows * c, dtype=np.uint64), p)).view(rows, c)
    rm = torch.ones(rows) if rowmask is None else rowmask
    dz = g * ((m * keep) * rm[:, None])
    dz64 = g.double() * m.double() * keep.double() * rm.double()[:, None]
    nblk = (rows + 63) // 64
    blocks = [slice(b * 64, min(b * 64 + 64, rows)) for b in range(nblk)]
    return SimpleNamespace(dz=dz, col64=dz64.sum(0), col32=dz.sum(0), part64=torch.stack([dz64[b].sum(0) for b in blocks]),
                           part32=torch.stack([dz[b].sum(0) for b in blocks]))


def _away(shape, gen):
    """random values with |v| >= 2e-3: no sign decision rests on a rounding"""
    v = torch.randn(shape, generator=gen)
    return torch.where(v >= 0, v + 2e-3, v - 2e-3)


@lru_cache(maxsize=8)
def act_inputs(rows, c, mode, masked, zeros=False):
    """g, y, x, rowmask, the start value of dbias and (modes 4, 5) the sign bytes.  y - x (mode 1) and y (modes 2, 3) stay 1e-3 away from 0.
    zeros: exact 0.0 and -0.0 planted in y (modes 1: y == x too; modes 2, 3) and in g (every mode); `planted` are their flat indices"""
    gen = _gen("act", rows, c, mode, masked, zeros)
    g = torch.randn(rows, c, generator=gen)
    x = y = ybytes = None
    if mode == 1:
        x = torch.randn(rows, c, generator=gen)
        d = _away((rows, c), gen)
        y = x + d
        bad = (y - x).abs() < 1e-3                    # the float32 sum moved y - x: take x = 0 there, where y - x = d exactly
        x = torch.where(bad, torch.zeros(()), x)
        y = torch.where(bad, d, y)
    elif mode in (2, 3):
        y = _away((rows, c), gen)
    elif mode in (4, 5):
        y = torch.rand(rows, c, generator=gen) > 0.5
        ybytes = sign_words(y) if mode == 4 else sign_bits(y)
    rm = (torch.rand(rows, generator=gen) > 0.25).float() if masked else None
    planted = None
    if zeros:
        n = rows * c
        planted = torch.randperm(n, generator=gen)[:64]
        if rm is not None:
            rm[planted[:48] // c] = 1.0                # (most of the planted elements in live rows)
        gf = g.view(-1)
        gf[planted[0:8]] = 0.0
        gf[planted[8:16]] = -0.0
        if mode in (1, 2, 3):
            yf = y.view(-1)
            if mode == 1:
                xf = x.view(-1)
                yf[planted[16:32]] = xf[planted[16:32]]                     # y == x
                xf[planted[32:40]] = 0.0
                yf[planted[32:40]] = -0.0                                   # 0 - (-0) and (-0) - 0
                xf[planted[40:48]] = -0.0
                yf[planted[40:48]] = 0.0
            else:
                yf[planted[16:32]] = 0.0
                yf[planted[32:48]] = -0.0
    db0 = torch.randn(c, generator=gen)
    return SimpleNamespace(g=g, y=y, x=x, rm=rm, db0=db0, ybytes=ybytes, planted=planted)


@lru_cache(maxsize=8)
def act_reference(rows, c, mode, masked, zeros=False, drop=None):
    i = act_inputs(rows, c, mode, masked, zeros)
    return act_bwd_ref(i.g, i.y, i.x, i.rm, ACT_SLOPE, mode, drop)


def act_reduction_cases():
    """(name, ref64, ref32) of every column-sum comparison of the GPU file: the atomic path onto db0 and the per-block rows"""
    for rows, c, masked, mode, zeros in act_cases():
        i, r = act_inputs(rows, c, mode, masked, zeros), act_reference(rows, c, mode, masked, zeros)
        name = f"{rows}x{c} mode={mode} mask={int(masked)}" + (" zeros" if zeros else "")
        yield f"dbias {name}", i.db0.double() + r.col64, i.db0 + r.col32
        for b in range(r.part64.shape[0]):
            yield f"parts[{b}] {name}", r.part64[b], r.part32[b]
    for rows, c, mode in act_dropout_cases():
        i = act_inputs(rows, c, mode, True)
        for drop in DROPS:
            r = act_reference(rows, c, mode, True, False, drop)
            yield f"dbias {rows}x{c} mode={mode} p={drop[0]} seed={drop[1]}", i.db0.double() + r.col64, i.db0 + r.col32


# ------------------------------------------------------------------------------------------------------------ split-K sum
def wgrad_reduce_ref(part, v=None, g=None):
    """part float32 [taps][nsplit][cout][cin] -> {"dw": (ref64, ref32)} [cout][cin][taps], and with weight norm (w = g v / ||v||)
    {"dg": ..., "dv": ...}: dg = <dW, v> / ||v||, dv = g / ||v|| (dW - v <dW, v> / ||v||^2)"""
    out = {}
    for i, dt in enumerate((torch.float64, torch.float32)):
        dw = part.to(dt).sum(1).permute(1, 2, 0).contiguous()
        res = {"dw": dw}
        if g is not None:
            vv, gg = v.to(dt), g.to(dt)
            dot, nn = (dw * vv).sum((1, 2)), (vv * vv).sum((1, 2))
            nrm = nn.sqrt()
            res["dg"] = dot / nrm
            res["dv"] = (gg / nrm)[:, None, None] * (dw - vv * (dot / nn)[:, None, None])
        for k, t in res.items():
            out.setdefault(k, [None, None])[i] = t
    return {k: tuple(t) for k, t in out.items()}


@lru_cache(maxsize=2)
def wgrad_inputs(cout, cin, taps, nsplit):
    """part ~ 0.1 N(0, 1), v ~ N(0, 1), g ~ U(0.5, 1.5): the inputs of tests/test_gpu_train.py"""
    gen = _gen("wgrad", cout, cin, taps, nsplit)
    part = 0.1 * torch.randn(taps, nsplit, cout, cin, generator=gen)
    v = torch.randn(cout, cin, taps, generator=gen)
    g = torch.rand(cout, generator=gen) + 0.5
    return part, v, g


@lru_cache(maxsize=2)
def wgrad_reference(cout, cin, taps, nsplit):
    part, v, g = wgrad_inputs(cout, cin, taps, nsplit)
    return wgrad_reduce_ref(part), wgrad_reduce_ref(part, v, g)


def wgrad_reduction_cases():
    for cout, cin, taps, nsplit, _ in WGRAD_CASES:
        plain, chain = wgrad_reference(cout, cin, taps, nsplit)
        name = f"{cout}x{cin}x{taps} nsplit={nsplit}"
        yield f"dw {name}", *plain["dw"]
        for k in ("dg", "dv"):
            yield f"{k} {name}", *chain[k]


def fold_reduction_cases():
    for cout, cin, taps in GROUPED_TILE_SHAPES + GROUPED_ROW_SHAPES:
        w, g = grouped_inputs(cout, cin, taps)
        for i in range(len(GROUPED_KINDS)):
            if GROUPED_KINDS[i][0]:
                yield f"fold {cout}x{cin}x{taps} item {i}", fold64(w[i], g[i]), fold(w[i], g[i], torch.float32)
