"""efts_gemm per tiling against float64 of its own operands  --  TEST INFRASTRUCTURE for tests/test_gemm_reference_cpu.py (no device)
and tests/test_gemm_kernels_gpu.py.  Plain module: importing it needs neither a GPU nor the library.

What is here:
  * host encoders of the three operand formats of include/efts_abi.h ("MFMA operand planes"); the decoder is kernel_check.unpack_plane;
  * the case table (CASES): the smallest shapes at which each of efts_gemm's kernels can still go wrong;
  * operands(case): inputs, ENCODED on the host -- the contraction tests do not depend on the pack kernels;
  * reference(case): the contraction and its epilogue in float64 and in float32, from the DECODED planes, i.e. from the exact numbers the
    kernel multiplies (operand rounding is not part of the error any more), and a rigorous per-element bound;
  * accepts(case, tiling): the dispatcher's documented rules (the comments at EFTS_TILING_* and the messages of efts_gemm).
"""
import math
import zlib
from dataclasses import dataclass
from functools import lru_cache
from types import SimpleNamespace

import torch

from kernel_check import unpack_plane

AUTO, GENERIC, WIDE, NARROW, RESIDENT, SMALLM = 0, 1, 2, 3, 4, 5            # EFTS_TILING_*
TILING_NAME = {AUTO: "auto", GENERIC: "generic", WIDE: "wide", NARROW: "narrow", RESIDENT: "resident", SMALLM: "smallm"}
EXPLICIT = (GENERIC, WIDE, NARROW, RESIDENT, SMALLM)
RING = (GENERIC, WIDE, NARROW, RESIDENT)                                    # bit-identical to each other and to AUTO (efts_abi.h `tiling`)
ACT_NONE, ACT_LEAKY, ACT_RELU, ACT_TANH = 0, 1, 2, 3                        # EFTS_ACT_*

A_GUARD_LO, A_GUARD_HI = 64, 144        # zero rows of the A plane in front of row 0 (the widest dilated halo is 32) and behind row m - 1
OUT_GUARD = 8                           # canary rows in front of and behind every output item
CANARY = 0x7F                           # every byte of an output before the launch: 0x7f7f7f7f = 3.39e38 as fp32, 0x7f7f as bf16 -- no result
TANH_ABS = 5e-7                         # tanhf of the device against tanh (tests/test_gpu_fp32.py::test_gemm_format3_activations_without_residual)
U = 2.0 ** -24                          # unit roundoff of fp32


def roundup(x, m):
    return (x + m - 1) // m * m


def chunk_k(split):
    """k's per 128-byte chunk"""
    return 64 if split == 1 else 32


def kp_of(K, split):
    return roundup(K, chunk_k(split))


def row_bytes(K, split):
    """bytes of a plane row that holds K values: nchunk * 128"""
    return kp_of(K, split) * (2 if split == 1 else 4)


def byte_offsets(k, split):
    """byte offsets inside a plane row of the number(s) that carry element k: (value,) for formats 1 and 3, (hi, lo) for format 2"""
    if split == 1:
        return (2 * k,)
    if split == 3:
        return (4 * k,)
    hi = (k // 32) * 128 + (k % 32) * 2
    return (hi, hi + 64)


def element_bytes(n, split, ld):
    """bool [ld]: the bytes of a plane row that belong to elements k < n"""
    mask = torch.zeros(ld, dtype=torch.bool)
    width = 4 if split == 3 else 2
    for k in range(n):
        for o in byte_offsets(k, split):
            mask[o:o + width] = True
    return mask


def encode_rows(x, split, ld=None, fill=0):
    """fp32 [rows][K] -> plane bytes uint8 [rows][ld]: the row, zero K padding up to Kp, then `fill` up to the row stride.
    bf16 = round to nearest even (torch's .bfloat16()); format 2: hi = bf16(x), lo = bf16(x - hi), 32 hi then 32 lo per chunk"""
    x = x.detach().float().contiguous()
    rows, K = x.shape
    kp = kp_of(K, split)
    xp = torch.zeros(rows, kp, dtype=torch.float32)
    xp[:, :K] = x
    if split == 3:
        raw = xp.view(torch.uint8)
    elif split == 1:
        raw = xp.bfloat16().view(torch.uint8)
    else:
        hi = xp.bfloat16()
        lo = (xp - hi.float()).bfloat16()
        raw = torch.stack((hi.view(rows, kp // 32, 32), lo.view(rows, kp // 32, 32)), 2).reshape(rows, 2 * kp).contiguous().view(torch.uint8)
    rb = raw.shape[1]
    assert rb == row_bytes(K, split)
    ld = rb if ld is None else ld
    assert ld >= rb
    out = torch.full((rows, ld), fill, dtype=torch.uint8)
    out[:, :rb] = raw
    return out


def encode_weight(w, split, ld=None, fill=0):
    """w fp32 [cout][cin][taps] (torch Conv1d layout) -> weight plane [taps][cout][ld]"""
    cout, cin, taps = w.shape
    return encode_rows(w.permute(2, 0, 1).reshape(taps * cout, cin), split, ld, fill).view(taps, cout, -1)


def decode_rows(plane, K, split, parts=False):
    """plane bytes [rows][ld] -> fp32 [rows][Kp] (parts: hi and lo)"""
    rows = plane.shape[0]
    r = unpack_plane(plane.contiguous(), 1, rows, rows, kp_of(K, split), split, parts=parts)
    return (r[0][0], r[1][0]) if parts else r[0]


def decode_weight(plane, cin, split, parts=False):
    """weight plane [taps][cout][ld] -> fp32 [taps][cout][Kp]"""
    taps, cout, ld = plane.shape
    r = decode_rows(plane.reshape(taps * cout, ld), cin, split, parts)
    if parts:
        return r[0].view(taps, cout, -1), r[1].view(taps, cout, -1)
    return r.view(taps, cout, -1)


# ------------------------------------------------------------------------------------------------------------ the cases
@dataclass(frozen=True)
class Case:
    name: str
    tilings: tuple          # explicit tilings the case is meant for: each of them must accept it
    refused: tuple = ()     # explicit tilings that must refuse it, by the design of the case
    split: int = 1
    taps: int = 1
    dil: int = 1
    m: int = 130
    n: int = 64
    K: int = 64
    batch: int = 1
    batch2: int = 1
    alpha: float = 1.0
    bias: bool = False
    act: int = ACT_NONE
    slope: float = 0.1
    resid: bool = False
    mask: bool = False
    items: tuple = ()       # (T, gap, len0, len1): a two-item row space, m = 2 * (T + gap); gap rows of A are zero, the mask is t < len
    out: str = "f32"        # "f32", "plane" or "both"
    ldo: int = 0            # 0: roundup(n, 4) + 4
    out_off: int = 0        # out_f32 moved by this many floats off its 16-byte alignment
    out_split: int = 0      # 0: the operand format
    plane_act: bool = False
    plane_slope: float = 0.2
    lo: bool = False        # out_bf16_lo

    @property
    def nchunk(self):
        return kp_of(self.K, self.split) // chunk_k(self.split)

    @property
    def pad(self):
        return (self.taps - 1) // 2

    @property
    def lda(self):
        return self.nchunk * 128 + 16

    @property
    def ldb(self):
        return self.nchunk * 128 + 32

    @property
    def has_f32(self):
        return self.out in ("f32", "both")

    @property
    def has_plane(self):
        return self.out in ("plane", "both")

    @property
    def ldo_(self):
        return (self.ldo or roundup(self.n, 4) + 4) if self.has_f32 else 0

    @property
    def ldr(self):
        return roundup(self.n, 4) + 8 if self.resid else 0

    @property
    def osplit(self):
        return self.out_split or self.split

    @property
    def ldob(self):
        return row_bytes(self.n, self.osplit) + 16 if self.has_plane else 0

    @property
    def vec_ok(self):
        """the float4 epilogue: 16-byte aligned fp32 rows, pointers and batch strides (the harness keeps residual and planes aligned)"""
        return not self.has_f32 or (self.ldo_ % 4 == 0 and self.out_off == 0)


def accepts(case, tiling):
    """does efts_gemm run `case` on `tiling`?  include/efts_abi.h at EFTS_TILING_* and the messages of efts_gemm"""
    c = case
    if tiling == AUTO:
        return True
    if c.split == 3:                                   # "split 3 (fp32) runs on the generic tiling only"
        return tiling == GENERIC
    if tiling == SMALLM:                               # "one dense 1 / 3 / 5-tap launch, n % 32 == 0, 16-byte aligned rows, plain outputs", batch 1
        return (c.batch == 1 and c.batch2 == 1 and c.dil == 1 and c.taps in (1, 3, 5) and c.n % 32 == 0 and not c.plane_act
                and c.act != ACT_TANH and not c.lo and c.vec_ok)
    if c.lo or c.batch2 > 1:                           # "out_bf16_lo / batch2 need the generic tiling"
        return tiling == GENERIC
    if tiling == GENERIC:                              # "every shape"
        return True
    if tiling == RESIDENT:                             # "n <= 64, one K chunk, taps 3 / 7 / 11"
        return c.n <= 64 and c.nchunk == 1 and c.taps in (3, 7, 11)
    if tiling == NARROW:                               # "no narrow instantiation for taps 9"
        return c.taps in (1, 3, 5, 7, 11)
    if tiling == WIDE:                                 # "dense k5 launches whose last 256-row window stays inside the guard rows", no tanh / plane_act
        mt = (c.m + 251) // 252
        return c.taps == 5 and c.dil == 1 and not c.plane_act and c.act != ACT_TANH and mt * 252 + 2 - c.m <= 144
    raise ValueError(tiling)


def _case(name, tilings, refused=(), items=None, **kw):
    if items:
        T, gap = items[0], items[1]
        kw["m"], kw["mask"] = 2 * (T + gap), True
    return Case(name=name, tilings=tuple(tilings), refused=tuple(refused), items=tuple(items or ()), **kw)


def _cases():
    G, W, N, R, S = GENERIC, WIDE, NARROW, RESIDENT, SMALLM
    tag = {1: "bf16", 2: "bf16x3", 3: "fp32"}
    out = []
    # ---- K steps against the 3-stage ring
    for sp in (1, 2):
        ck = chunk_k(sp)
        for nc in (1, 2, 3, 4):
            out.append(_case(f"k-{tag[sp]}-t1-nc{nc}", (G, N, S), split=sp, K=nc * ck, bias=True))
        out.append(_case(f"k-{tag[sp]}-t3-nc1", (G, N, R, S), split=sp, taps=3, K=ck, bias=True))
        for K in (24, 80, 130):
            out.append(_case(f"k-{tag[sp]}-t1-K{K}", (G, N, S), split=sp, K=K, bias=True))
        out.append(_case(f"k-{tag[sp]}-t5-K320", (G, W, N, S), split=sp, taps=5, K=320, bias=True))
    for nc in (1, 2, 3, 4):
        out.append(_case(f"k-bf16-t5-nc{nc}", (G, W, N, S), taps=5, K=64 * nc, bias=True))
    for nc in (1, 2, 3, 4):
        out.append(_case(f"k-fp32-t1-nc{nc}", (G,), split=3, K=32 * nc, bias=True))
    out.append(_case("k-fp32-t3-nc1", (G,), split=3, taps=3, K=32, bias=True))
    for K in (24, 130):
        out.append(_case(f"k-fp32-t1-K{K}", (G,), split=3, K=K, bias=True))
    # ---- row edges, every kernel on its own BM
    edge = dict(bias=True, resid=True, mask=True, out="both")
    for sp in (1, 2):
        for m in (1, 123, 124, 125, 249):                  # generic / narrow, taps 5: BM = 124
            out.append(_case(f"row-{tag[sp]}-t5-m{m}", (G, N), split=sp, taps=5, m=m, n=96, K=64, **edge))
    for sp, ms in ((1, (1, 253, 254, 255, 509)), (2, (254, 255, 509))):      # resident, taps 3: BM = 254
        for m in ms:
            out.append(_case(f"row-{tag[sp]}-t3-m{m}", (G, N, R), split=sp, taps=3, m=m, n=32, K=chunk_k(sp), **edge))
    for sp, ms in ((1, (63, 64, 65, 129)), (2, (65, 129))):                  # small-M: BM = 64
        for m in ms:
            out.append(_case(f"row-{tag[sp]}-smallm-m{m}", (G, N, S), split=sp, taps=5, m=m, n=32, K=2 * chunk_k(sp), **edge))
    for sp, ms in ((1, (110, 252, 362, 504)), (2, (362,))):                  # wide: BM = 252; the smallest / largest m whose last window fits
        for m in ms:
            out.append(_case(f"row-{tag[sp]}-wide-m{m}", (G, W), split=sp, taps=5, m=m, n=128, K=64, **edge))
    for m in (109, 253):
        out.append(_case(f"row-bf16-wide-m{m}-refused", (G,), (W,), taps=5, m=m, n=128, K=64, **edge))
    # ---- column edges
    for sp, ns in ((1, (4, 28, 32, 36, 60, 64, 68, 96, 124, 128, 132)), (2, (36, 64, 132))):
        for n in ns:
            out.append(_case(f"col-{tag[sp]}-t5-n{n}", (G, W, N) + ((S,) if n % 32 == 0 else ()), () if n % 32 == 0 else (S,),
                             split=sp, taps=5, n=n, K=64, **edge))
    for sp in (1, 2):
        out.append(_case(f"col-{tag[sp]}-t5-n130-ldo130", (G, W, N), (S,), split=sp, taps=5, n=130, ldo=130, K=64, **edge))      # scalar throughout
    out.append(_case("col-bf16-t5-n130-ldo132", (G, W, N), (S,), taps=5, n=130, ldo=132, K=64, **edge))         # vector body + scalar tail
    out.append(_case("col-bf16-t5-n64-unaligned", (G, W, N), (S,), taps=5, n=64, ldo=64, out_off=1, K=64, **edge))   # vec_ok false, aligned shape
    for n in (4, 28, 32, 36, 60, 64):
        out.append(_case(f"col-bf16-t3-n{n}", (G, N, R), taps=3, n=n, K=64, **edge))
    out.append(_case("col-bf16-t3-n30-ldo30", (G, N, R), (S,), taps=3, n=30, ldo=30, K=64, **edge))
    out.append(_case("col-bf16-t3-n64-unaligned", (G, N, R), (S,), taps=3, n=64, ldo=64, out_off=1, K=64, **edge))
    out.append(_case("col-bf16x3-t3-n36", (G, N, R), (S,), split=2, taps=3, n=36, K=32, **edge))
    out.append(_case("col-bf16x3-t3-n30-ldo30", (G, N, R), (S,), split=2, taps=3, n=30, ldo=30, K=32, **edge))
    # ---- taps and dilation on a two-item row space with a ragged second item
    conv = dict(bias=True, resid=True, out="both")
    for sp, ts in ((1, (1, 3, 5, 7, 9, 11)), (2, (9, 11))):
        for t in ts:
            til = (G,) if t == 9 else (G, N)
            out.append(_case(f"taps-{tag[sp]}-t{t}", til, (N,) if t == 9 else (), items=(70, max(2, (t - 1) // 2), 70, 33),
                             split=sp, taps=t, n=64, K=chunk_k(sp), **conv))
    for sp in (1, 2):
        for t, d in ((3, 1), (7, 3), (11, 5), (11, 6), (3, 32)):          # (11, 6): (taps - 1) * dil = 60; (3, 32): exactly 64
            out.append(_case(f"dil-{tag[sp]}-t{t}-d{d}", (G, N, R), items=(150, (t - 1) // 2 * d, 150, 113),
                             split=sp, taps=t, dil=d, n=48, K=chunk_k(sp), **conv))
    out.append(_case("dil-bf16-t5-d16", (G, N), items=(150, 32, 150, 113), taps=5, dil=16, n=48, K=64, **conv))
    # ---- epilogue terms, one at a time, on a k5 shape (generic, wide, narrow, small-M) and a k3 shape (generic, narrow, resident, small-M)
    for t, til in ((5, (G, W, N, S)), (3, (G, N, R, S))):
        base = dict(taps=t, m=130, n=64, K=64)
        ring = tuple(x for x in til if x != S)
        e = f"epi-bf16-t{t}"
        out.append(_case(f"{e}-plain", til, **base))
        out.append(_case(f"{e}-alpha", til, alpha=0.125, **base))
        out.append(_case(f"{e}-bias", til, bias=True, **base))
        out.append(_case(f"{e}-leaky", til, bias=True, act=ACT_LEAKY, **base))
        out.append(_case(f"{e}-relu", til, bias=True, act=ACT_RELU, **base))
        out.append(_case(f"{e}-tanh", tuple(x for x in ring if x != W), (S,) + ((W,) if W in til else ()), bias=True, act=ACT_TANH, **base))
        out.append(_case(f"{e}-resid", til, resid=True, **base))
        out.append(_case(f"{e}-mask", til, mask=True, **base))
        out.append(_case(f"{e}-plane-only", til, bias=True, out="plane", **base))
        out.append(_case(f"{e}-both-os1", til, bias=True, out="both", out_split=1, **base))
        out.append(_case(f"{e}-both-os2", til, bias=True, out="both", out_split=2, **base))
        out.append(_case(f"{e}-plane-act", tuple(x for x in ring if x != W), (S,) + ((W,) if W in til else ()), bias=True, out="both", plane_act=True, **base))
        out.append(_case(f"{e}-lo", (G,), tuple(x for x in til if x != G), bias=True, out="both", out_split=1, lo=True, **base))
        out.append(_case(f"{e}-all", til, alpha=0.125, bias=True, act=ACT_LEAKY, resid=True, mask=True, out="both", **base))
        base2 = dict(base, split=2, K=32)
        e = f"epi-bf16x3-t{t}"
        out.append(_case(f"{e}-both-os1", til, bias=True, out="both", out_split=1, **base2))
        out.append(_case(f"{e}-both-os2", til, bias=True, out="both", out_split=2, **base2))
        out.append(_case(f"{e}-all", til, alpha=0.125, bias=True, act=ACT_LEAKY, resid=True, mask=True, out="both", **base2))
    out.append(_case("epi-fp32-t3-all", (G,), split=3, taps=3, m=130, n=64, K=32, alpha=0.125, bias=True, act=ACT_LEAKY, resid=True, mask=True,
                     out="both", plane_act=True))
    # ---- batching: strides that are not the dense ones, the outer batch, a tile count that is no multiple of 8
    for sp in (1, 2):
        out.append(_case(f"batch-{tag[sp]}-t3-b3", (G, N, R), (S,), split=sp, taps=3, m=130, n=64, K=chunk_k(sp), batch=3, bias=True, resid=True,
                         mask=True, out="both"))
    out.append(_case("batch2-bf16-t1-b3", (G,), (W, N, R, S), taps=1, m=130, n=64, K=80, batch2=3, alpha=0.125))
    out.append(_case("batch-bf16-t1-b2-ntot9", (G, N), (S,), taps=1, m=300, n=384, K=64, batch=2, bias=True, mask=True))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


CASES = _cases()


# ------------------------------------------------------------------------------------------------------------ operands
@lru_cache(maxsize=4)
def operands(case):
    """inputs of `case`: fp32 tensors and the planes ENCODED from them on the host.
    A: uint8 [batch2 * batch][64 + m + 144][lda]  (zero guard rows; the stride padding of every row holds CANARY: never read)
    B: uint8 [batch2 * batch][taps * n + 1][ldb]  (one spare row per item: the batch stride is not the dense one)
    bias [n]; resid [batch][m + 2][ldr]; rowmask [batch][m + 3]"""
    c = case
    g = torch.Generator().manual_seed(zlib.crc32(c.name.encode()))
    nb = c.batch2 * c.batch
    x = torch.randn(nb, c.m, c.K, generator=g)
    w = torch.randn(nb, c.n, c.K, c.taps, generator=g) / math.sqrt(c.K * c.taps)
    bias = torch.randn(c.n, generator=g)
    resid = torch.randn(c.batch, c.m + 2, max(c.ldr, 1), generator=g)
    mask = (torch.rand(c.batch, c.m + 3, generator=g) > 0.25).float()
    if c.items:
        T, gap, l0, l1 = c.items
        t = torch.arange(c.m) % (T + gap)
        x[:, t >= T] = 0.0
        mask[:, :c.m] = (t < torch.tensor([l0] * (T + gap) + [l1] * (T + gap))).float()
    ra = A_GUARD_LO + c.m + A_GUARD_HI
    a_pl = torch.zeros(nb, ra, c.lda, dtype=torch.uint8)
    a_pl[:, :, c.nchunk * 128:] = CANARY
    b_pl = torch.full((nb, c.taps * c.n + 1, c.ldb), CANARY, dtype=torch.uint8)
    for i in range(nb):
        a_pl[i, A_GUARD_LO:A_GUARD_LO + c.m] = encode_rows(x[i], c.split, c.lda, CANARY)
        b_pl[i, :c.taps * c.n] = encode_weight(w[i], c.split, c.ldb, CANARY).view(c.taps * c.n, c.ldb)
    return SimpleNamespace(x=x, w=w, bias=bias, resid=resid, mask=mask, a=a_pl, b=b_pl)


def _leaky(v, slope):
    return torch.where(v > 0, v, v * slope)


def _ulp(v):
    """an upper bound of the spacing of fp32 at v"""
    return v.abs() * 2.0 ** -23 + 2.0 ** -149


@lru_cache(maxsize=4)
def reference(case, plane=False):
    """(ref64, ref32, bound), each [batch2][batch][m][n], of the fp32 output -- or, with plane, of the value the plane output encodes.
    Computed from the DECODED planes.  Format 2 sums the three products the kernel sums: hi*hi + hi*lo + lo*hi.
    bound: n_terms * 2^-24 * sum |a||b| (any summation order of fp32 additions of the exact products), scaled by |alpha|, plus one ulp of
    the running value per epilogue step (every step is 1-Lipschitz, so earlier errors do not grow), plus TANH_ABS for tanhf."""
    c = case
    op = operands(c)
    nb = c.batch2 * c.batch
    kp = kp_of(c.K, c.split)
    n_terms = c.taps * kp * (3 if c.split == 2 else 1)           # products accumulated per output element
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))  # the scalars as the kernel holds them
    alpha, slope, pslope = f32(c.alpha), f32(c.slope), f32(c.plane_slope)
    res = {torch.float64: [], torch.float32: []}
    bounds = []
    for i in range(nb):
        ah, al = decode_rows(op.a[i, A_GUARD_LO:A_GUARD_LO + c.m], c.K, c.split, parts=True)          # rows outside [0, m) are zero
        wh, wl = decode_weight(op.b[i, :c.taps * c.n].view(c.taps, c.n, c.ldb), c.K, c.split, parts=True)
        z = i % c.batch
        for dt in (torch.float64, torch.float32):
            A = [torch.nn.functional.pad(t.to(dt), (0, 0, A_GUARD_LO, A_GUARD_HI)) for t in (ah, al)]
            Wt = [t.to(dt) for t in (wh, wl)]
            s = torch.zeros(c.m, c.n, dtype=dt)
            mag = torch.zeros(c.m, c.n, dtype=dt)
            for k in range(c.taps):
                r0 = A_GUARD_LO + (k - c.pad) * c.dil
                h, l = A[0][r0:r0 + c.m], A[1][r0:r0 + c.m]
                s = s + h @ Wt[0][k].T
                mag = mag + h.abs() @ Wt[0][k].abs().T
                if c.split == 2:
                    s = s + h @ Wt[1][k].T + l @ Wt[0][k].T
                    mag = mag + h.abs() @ Wt[1][k].abs().T + l.abs() @ Wt[0][k].abs().T
            err = abs(alpha) * n_terms * U * mag
            v = alpha * s
            err = err + _ulp(v)
            if c.bias:
                v = v + op.bias.to(dt)
                err = err + _ulp(v)
            if c.act == ACT_LEAKY:
                v = _leaky(v, slope)
                err = err + _ulp(v)
            elif c.act == ACT_RELU:
                v = torch.relu(v)
            elif c.act == ACT_TANH:
                v = torch.tanh(v)
                err = err + _ulp(v) + TANH_ABS
            if c.resid:
                v = v + op.resid[z, :c.m, :c.n].to(dt)
                err = err + _ulp(v)
            if c.mask:
                v = v * op.mask[z, :c.m, None].to(dt)
                err = err * op.mask[z, :c.m, None].to(dt)
            if plane and c.plane_act:
                v = _leaky(v, pslope)
                err = err + _ulp(v)
            res[dt].append(v)
            if dt == torch.float64:
                bounds.append(err)
    shape = (c.batch2, c.batch, c.m, c.n)
    return (torch.stack(res[torch.float64]).view(shape), torch.stack(res[torch.float32]).view(shape), torch.stack(bounds).view(shape))


def storage_resolution(split):
    """what decoding a plane of format `split` adds to an error, relative: `extra` of kernel_check._check"""
    return {1: 2.0 ** -8, 2: 2.0 ** -16, 3: 0.0}[split]
