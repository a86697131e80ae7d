"""Train-mode Dropout of every launch that draws its own mask, on the host  --  TEST INFRASTRUCTURE for
tests/test_dropout_reference_cpu.py (no device) and tests/test_dropout_kernels_gpu.py.  Plain module: importing it needs neither a GPU
nor the library.

No launch stores a mask: each draws it from (seed, element index) with drop_scale(hash_u32(seed), index, thresh, inv_keep) of
csrc/efts_internal.h, and the backward launch draws it again.  The numpy transcription of that mixer is train_pack_reference's
(hash_u32, drop_params, keep_scale), pinned to the header by test_keep_scale_hash_is_the_headers_mixer; nothing here mixes bits itself.

What is here:
  * ln_keep_scale: the LayerNorm launches hash `drop_seed + *drop_seed_add` (uint32, on the device);
  * GEMM_CASES / gemm_reference: efts_gemm with drop_p > 0 on gemm_reference.Case, operands and reference -- the activated value of the
    decoded planes, times keep_scale, THEN residual and row mask;
  * LN_CASES / ln_inputs / ln_forward / ln_backward: efts_layernorm_rows, efts_layernorm_dot (mode 0 and 1) and efts_layernorm_bwd (forms
    dy, ddur, ddur_rowmask): the mask on LN * gamma + beta, before the row mask or the dot; the backward is torch autograd of that;
  * act_cases / act_inputs / act_forward / act_backward: efts_act_apply and efts_act_grad: the mask on f(z), before the residual;
  * reduction_cases: every sum the GPU file holds to kernel_check._check, for the CPU file to assert the condition of the bound on.
Every reference is a (float64, float32) pair of the same transcription.
"""
import dataclasses
import zlib
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import torch

import bwd_reference as B
import fwd_cases as F
import gemm_reference as G
from train_pack_reference import _away, keep_scale

DROP_PS = (0.1, 0.25, 0.5)
DROP_SEEDS = (77, 0x9E3779B9)                     # the second one is >= 2^31
DROPS = tuple((p, s) for p in DROP_PS for s in DROP_SEEDS)
LN_EPS = 1e-12
DOT_OFFSET = 1.0


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def ln_keep_scale(seed, add, idx, p):
    """the mask of efts_layernorm_rows / _dot / _bwd: the device adds the word behind drop_seed_add to drop_seed in uint32 and hashes the sum"""
    return keep_scale((int(seed) + int(add or 0)) & 0xFFFFFFFF, idx, p)


def _mask2d(ks_fn, rows, c):
    return torch.from_numpy(ks_fn(np.arange(rows * c, dtype=np.uint64))).view(rows, c)


# ------------------------------------------------------------------------------------------------------------ efts_gemm
@dataclasses.dataclass(frozen=True)
class GemmDrop:
    case: G.Case
    p: float
    seed: int
    tilings: tuple          # the tilings the GPU file launches (each accepts the case); AUTO is among them
    sign: bool              # sign_mask too (n % 128 == 0)

    @property
    def name(self):
        return self.case.name

    @property
    def plain(self):
        """the same contraction without residual, row mask (and dropout): what the kernel activates"""
        return dataclasses.replace(self.case, resid=False, mask=False, out="f32")


def _gemm_cases():
    s0, s1 = DROP_SEEDS
    GA, GWA = (G.GENERIC, G.AUTO), (G.GENERIC, G.WIDE, G.AUTO)
    # (taps, m, n, split, ldo - n, p, seed).  m = 130, one tap: two row tiles of 128.  m = 362, five taps: three generic row tiles of 124,
    # two wide ones of 252, the largest overhang the wide tiling accepts.  n = 256: the column-tile offset enters the index; 320: a partial
    # third tile; 80: n % 128 != 0.  ldo = n + 8: the index uses n, not the row stride.  Split 3 (fp32 planes): the generic tiling, one tap
    table = (
        (5, 362, 128, 1, 0, 0.25, s0), (5, 362, 128, 2, 8, 0.5, s1), (5, 362, 256, 1, 8, 0.5, s0), (5, 362, 256, 2, 0, 0.1, s1),
        (5, 362, 320, 1, 0, 0.1, s1), (5, 362, 320, 2, 8, 0.25, s0), (5, 362, 80, 1, 8, 0.5, s1), (5, 362, 80, 2, 0, 0.25, s0),
        (1, 130, 128, 1, 0, 0.5, s1), (1, 130, 256, 1, 8, 0.1, s0), (1, 130, 256, 2, 0, 0.25, s1), (1, 130, 320, 2, 0, 0.5, s0),
        (1, 130, 80, 2, 8, 0.1, s1), (1, 130, 128, 3, 8, 0.25, s1), (1, 130, 256, 3, 0, 0.5, s0), (1, 130, 320, 3, 8, 0.1, s0),
        (1, 130, 80, 3, 0, 0.5, s1), (1, 7, 128, 1, 0, 0.25, s0), (5, 7, 320, 2, 8, 0.5, s1), (1, 7, 80, 3, 0, 0.1, s0),
    )
    tag = {1: "bf16", 2: "bf16x3", 3: "fp32"}
    out = []
    for taps, m, n, sp, dldo, p, seed in table:
        wide = taps == 5 and m == 362 and sp != 3
        tilings = GWA if wide else GA
        name = f"drop-{tag[sp]}-t{taps}-m{m}-n{n}-ldo{n + dldo}-p{p}-s{seed}"
        case = G.Case(name=name, tilings=tuple(t for t in tilings if t != G.AUTO), split=sp, taps=taps, m=m, n=n, K=G.chunk_k(sp), batch=1, bias=True,
                      act=G.ACT_LEAKY, resid=True, mask=True, out="both", ldo=n + dldo)
        assert all(G.accepts(case, t) for t in tilings)
        out.append(GemmDrop(case=case, p=p, seed=seed, tilings=tilings, sign=n % 128 == 0))
    assert len({d.name for d in out}) == len(out)
    return tuple(out)


GEMM_CASES = _gemm_cases()
GEMM_PAIR_CASE = next(d for d in GEMM_CASES if d.case.m == 130 and d.case.n == 256 and d.case.split == 1)   # the smallest with 2 x 2 tiles


def gemm_keep(d, seed=None):
    """float32 [m][n]: keep_scale(seed, row * n + col, p)"""
    c = d.case
    return _mask2d(lambda idx: keep_scale(d.seed if seed is None else seed, idx, d.p), c.m, c.n)


@lru_cache(maxsize=2)
def gemm_reference(d):
    """efts_gemm with dropout from the DECODED planes: ((act(alpha a.b + bias)) * keep + resid) * rowmask in float64 and float32, and the
    a-priori bound of gemm_reference.reference carried through the three extra steps (each rounds once; every step is at most
    inv_keep-Lipschitz, and the bound is scaled by it).  keep [m][n] float32, resid [m][n], mask [m]"""
    c = d.case
    a64, a32, ab = (t[0, 0] for t in G.reference(d.plain))
    op = G.operands(c)
    resid, mask = op.resid[0, :c.m, :c.n], op.mask[0, :c.m]
    keep = gemm_keep(d)
    k64 = keep.double()
    v64 = a64 * k64
    bound = ab * k64 + G._ulp(v64)
    v64 = v64 + resid.double()
    bound = (bound + G._ulp(v64)) * mask.double()[:, None]
    ref64 = v64 * mask.double()[:, None]
    ref32 = (a32 * keep + resid) * mask[:, None]
    return SimpleNamespace(ref64=ref64, ref32=ref32, bound=bound, a64=a64, a32=a32, keep=keep, resid=resid, mask=mask)


# ------------------------------------------------------------------------------------------------------------ LayerNorm
# (rows, c, p, seed, seed_add).  Forward blocks hold 4 rows, backward blocks 8: rows 1, 7, 9, 130.  seed_add None: no device word
WRAP_ADD = 0x7FFFFFFF                             # with seed 0x9E3779B9 the uint32 sum wraps past 2^32
LN_CASES = (
    (1, 256, 0.5, DROP_SEEDS[0], None), (7, 256, 0.1, DROP_SEEDS[1], 5), (9, 256, 0.25, DROP_SEEDS[0], 0xFFFF0000), (130, 256, 0.5, DROP_SEEDS[1], WRAP_ADD),
    (1, 512, 0.1, DROP_SEEDS[1], 1234567), (7, 512, 0.25, DROP_SEEDS[0], None), (9, 512, 0.5, DROP_SEEDS[1], WRAP_ADD), (130, 512, 0.1, DROP_SEEDS[0], 3),
    (1, 2048, 0.25, DROP_SEEDS[1], WRAP_ADD), (7, 2048, 0.5, DROP_SEEDS[0], 40000), (9, 2048, 0.1, DROP_SEEDS[1], None), (130, 2048, 0.25, DROP_SEEDS[0], 1),
)
LN_FORMS = ("dy", "ddur", "ddur_rowmask")
LN_PAIR_CASE = LN_CASES[2]                        # 9 x 256: three forward blocks, two backward blocks, a device word
LN_STREAM_CASE = LN_CASES[1]


def ln_id(case):
    rows, c, p, seed, add = case
    return f"{rows}x{c}-p{p}-s{seed}-add{add}"


@lru_cache(maxsize=4)
def ln_inputs(rows, c):
    """z (the kernel gets x = relu(z)), gamma, a beta away from 0, a row mask with dead rows, the Linear(c, 1) w and b, the two upstream
    gradients (ddur is 0 on dead rows, as efts_loss_bwd leaves it) and the start values of the accumulated gradients"""
    g = _gen("ln", rows, c)
    z = torch.randn(rows, c, generator=g)
    gamma = 1.0 + 0.1 * torch.randn(c, generator=g)
    beta = 0.1 * _away((c,), g)                                                       # no beta is 0
    rm = (torch.rand(rows, generator=g) > 0.3).float()
    if rows > 1:
        rm[0], rm[rows - 1] = 1.0, 0.0
    w, b = torch.randn(c, generator=g) / c ** 0.5, torch.randn(1, generator=g)
    dy = _away((rows, c), g)
    ddur = (0.5 + torch.randn(rows, generator=g)) * rm            # (around 0.5: see test_layernorm_bwd_vs_fp64 on the conditioning of db)
    init = {k: torch.randn(c if k != "db" else 1, generator=g) for k in ("dgamma", "dbeta", "dbias", "dw", "db")}
    return SimpleNamespace(z=z, x=torch.relu(z), gamma=gamma, beta=beta, rm=rm, w=w, b=b, dy=dy, ddur=ddur, init=init)


def ln_keep(case, add="case"):
    rows, c, p, seed, a = case
    return _mask2d(lambda idx: ln_keep_scale(seed, a if add == "case" else add, idx, p), rows, c)


def _ln_masked(i, keep, dtype, leaves=False):
    t = lambda v: v.to(dtype)                                                         # noqa: E731
    z, bias = t(i.z), torch.zeros(i.z.shape[1], dtype=dtype)
    gm, bt, ww, bb = t(i.gamma), t(i.beta), t(i.w), t(i.b)
    if leaves:
        z, bias, gm, bt, ww, bb = (v.requires_grad_(True) for v in (z, bias, gm, bt, ww, bb))
    y = B.relu_layernorm(z + bias, gm, bt, LN_EPS) * t(keep)                          # Dropout on LN * gamma + beta, before the row mask or the dot
    return y, (z, gm, bt, bias, ww, bb)


@lru_cache(maxsize=4)
def ln_forward(case, add="case"):
    """{"rows": y * rowmask, "dot0": (y . w + b) * rowmask, "dot1": max(exp(y . w + b) - offset, 0) * rowmask}, each (float64, float32)"""
    i, keep = ln_inputs(case[0], case[1]), ln_keep(case, add)
    out = {}
    for dt in (torch.float64, torch.float32):
        y, (_, _, _, _, ww, bb) = _ln_masked(i, keep, dt)
        rm = i.rm.to(dt)
        dot = y @ ww + bb
        res = dict(rows=y * rm[:, None], dot0=dot * rm, dot1=torch.clamp(torch.exp(dot) - DOT_OFFSET, min=0.0) * rm)
        for k, v in res.items():
            out.setdefault(k, []).append(v)
    return {k: tuple(v) for k, v in out.items()}


@lru_cache(maxsize=4)
def ln_backward(case, form):
    """float64 / float32 autograd of the masked forward: {"dz", "dgamma", "dbeta", "dbias"[, "dw", "db"]}, the sums on top of their start
    values.  dy: <y * rowmask, dy>; ddur, ddur_rowmask: <y . w + b, ddur> (the kernel's rowmask then only multiplies dz, where ddur is 0)"""
    i, keep = ln_inputs(case[0], case[1]), ln_keep(case)
    out = {}
    for dt in (torch.float64, torch.float32):
        y, (z, gm, bt, bias, ww, bb) = _ln_masked(i, keep, dt, leaves=True)
        init = {k: v.to(dt) for k, v in i.init.items()}
        if form == "dy":
            loss = (y * i.rm.to(dt)[:, None] * i.dy.to(dt)).sum()
            gz, ggm, gbt, gbias = torch.autograd.grad(loss, (z, gm, bt, bias))
            res = dict(dz=gz, dgamma=init["dgamma"] + ggm, dbeta=init["dbeta"] + gbt, dbias=init["dbias"] + gbias)
        else:
            loss = ((y @ ww + bb) * i.ddur.to(dt)).sum()
            gz, ggm, gbt, gbias, gw, gb = torch.autograd.grad(loss, (z, gm, bt, bias, ww, bb))
            res = dict(dz=gz, dgamma=init["dgamma"] + ggm, dbeta=init["dbeta"] + gbt, dbias=init["dbias"] + gbias, dw=init["dw"] + gw, db=init["db"] + gb)
        for k, v in res.items():
            out.setdefault(k, []).append(v)
    return {k: tuple(v) for k, v in out.items()}


# ------------------------------------------------------------------------------------------------------------ efts_act_apply / efts_act_grad
ACT_NAMES = ("SiLU", "Tanh", "LeakyReLU", "Identity")            # one smooth, one saturating, one piecewise, Identity
ACT_PAIR_SHAPE = (65, 132)                                        # two 64-row blocks, two 128-column groups


def act_cases():
    """(name, params, rows, c, p, seed): the four activations of fwd_cases.act_list() on fwd_cases.ACT_SHAPES, the (p, seed) pairs dealt round"""
    acts = [(n, p) for n, p in F.act_list() if n in ACT_NAMES]
    assert sorted(n for n, _ in acts) == sorted(ACT_NAMES)
    out = []
    for a, (name, params) in enumerate(acts):
        for s, (rows, c) in enumerate(F.ACT_SHAPES):
            p, seed = DROPS[(a * len(F.ACT_SHAPES) + s) % len(DROPS)]
            out.append((name, params, rows, c, p, seed))
    return out


def act_case_id(case):
    name, params, rows, c, p, seed = case
    return f"{F.act_id(name, params)}-{rows}x{c}-p{p}-s{seed}"


@lru_cache(maxsize=4)
def act_inputs(rows, c):
    """z and the upstream gradient away from 0 (f(z) and f'(z) of the four activations are then non-zero), a residual, a row mask with
    dead rows, the start value of dbias"""
    g = _gen("act", rows, c)
    z = _away((rows, c), g)
    up = _away((rows, c), g)
    resid = torch.randn(rows, c, generator=g)
    rm = (torch.rand(rows, generator=g) > 0.3).float()
    if rows > 1:
        rm[0], rm[rows - 1] = 1.0, 0.0
    db0 = torch.randn(c, generator=g)
    return SimpleNamespace(z=z, up=up, resid=resid, rm=rm, db0=db0)


def act_keep(case, seed=None):
    _, _, rows, c, p, s = case
    return _mask2d(lambda idx: keep_scale(s if seed is None else seed, idx, p), rows, c)


def _act_key(case):
    name, params, rows, c, p, seed = case
    return name, tuple(sorted(params.items())), rows, c, p, seed


@lru_cache(maxsize=8)
def _act_reference(key, use_resid, use_mask):
    name, params, rows, c, p, seed = key
    i = act_inputs(rows, c)
    keep = _mask2d(lambda idx: keep_scale(seed, idx, p), rows, c)
    mod = getattr(torch.nn, name)(**dict(params))
    out = {}
    for dt in (torch.float64, torch.float32):
        z = i.z.to(dt).requires_grad_(True)
        v = mod(z) * keep.to(dt)                                                      # Dropout on f(z), before the residual
        if use_resid:
            v = v + i.resid.to(dt)
        y = v * i.rm.to(dt)[:, None] if use_mask else v
        (dz,) = torch.autograd.grad((y * i.up.to(dt)).sum(), z)
        for k, t in (("y", y.detach()), ("dz", dz), ("dbias", i.db0.to(dt) + dz.sum(0))):
            out.setdefault(k, []).append(t)
    return {k: tuple(v) for k, v in out.items()}


def act_reference(case, use_resid, use_mask):
    """{"y": (resid + f(z) * keep) * rowmask, "dz": torch autograd of <y, up>, "dbias": db0 + column sums of dz}, each (float64, float32)"""
    return _act_reference(_act_key(case), use_resid, use_mask)


# ------------------------------------------------------------------------------------------------------------ what the CPU file walks
def reduction_cases():
    """(name, ref64, ref32) of every sum the GPU file holds to kernel_check._check"""
    for case in LN_CASES:
        fwd = ln_forward(case)
        for k in ("dot0", "dot1"):
            yield f"efts_layernorm_dot.{k} {ln_id(case)}", *fwd[k]
        for form in LN_FORMS:
            r = ln_backward(case, form)
            for k in ("dgamma", "dbeta", "dbias", "dw", "db"):
                if k in r:
                    yield f"efts_layernorm_bwd.{k} {form} {ln_id(case)}", *r[k]
    for case in act_cases():
        for use_mask in (False, True):
            yield f"efts_act_grad.dbias {act_case_id(case)} mask={int(use_mask)}", *act_reference(case, True, use_mask)["dbias"]


def mask_cases():
    """(name, p, keep [rows][c] float32) of every case's host mask (the LayerNorm ones with their device word applied)"""
    for d in GEMM_CASES:
        yield d.name, d.p, gemm_keep(d)
    for case in LN_CASES:
        yield "ln " + ln_id(case), case[2], ln_keep(case)
    for case in act_cases():
        yield "act " + act_case_id(case), case[4], act_keep(case)
