"""Inputs and float64 / float32 references of the forward single-kernel tests  --  TEST INFRASTRUCTURE.

tests/test_fwd_kernels_gpu.py and tests/test_act_kernels_gpu.py run a kernel on what a maker below returns and compare it with the
`refs` of the same call; tests/test_fwd_reference_cpu.py walks every case without a device and asserts the condition of the bound
(kernel_check.conditioned) on the same `refs`.  One definition, so the conditioning that was checked is the conditioning that runs.

Every maker returns a dict whose `refs` maps an output name to (float64 reference, float32 transcription).  Kernel and reference
get the same float32 inputs; a stage input (IMV, e) is computed in float64 from the primary input and rounded to float32.
Plain module, no GPU, no library.
"""
import torch

import bwd_reference as R

SIGMA, SIGMA_E, OFFSET = 0.01, 0.5, 1.0

ATTN_SHAPES = [(3, 1, 33), (3, 5, 64), (4, 9, 33), (3, 37, 211), (2, 63, 97), (2, 64, 130), (2, 65, 70), (2, 203, 300)]
IMV_T2 = [1, 2, 63, 64, 65, 127, 128, 129, 211, 800, 4100]
IMV_T1 = 40
EPOS_SHAPES = ATTN_SHAPES + [(2, 128, 800), (2, 203, 1500)]
DUR_SHAPES = [(3, 1), (3, 5), (4, 37), (2, 203)]
ALIGN_SHAPES = [(3, 37, 211), (2, 128, 800), (4, 100, 124), (1, 9, 33), (2, 200, 1500), (2, 128, 4100), (3, 1, 33), (2, 203, 1500)]
RALPHA_SHAPES = [(3, 37, 211), (4, 16, 31), (2, 31, 64), (2, 33, 65), (2, 256, 70), (2, 300, 333), (1, 1, 5)]
CHAIN_SHAPES = [(3, 37, 211), (2, 128, 800)]


def lengths(B, T1, T2, seed):
    """ragged; item 0 spans both padded lengths, the last item has text_len 1 and (B >= 3) item 1 has mel_len 1"""
    g = torch.Generator().manual_seed(seed)
    tl = R.ragged_lengths(B, T1, g, last=1)
    ml = R.ragged_lengths(B, T2, g)
    if B >= 3:
        ml[1] = 1
    return g, tl, ml


def _pair(fn, *xs):
    """(fn in float64, fn in float32) of float32 inputs"""
    return fn(*[x.double() for x in xs]), fn(*xs)


def attn_case(B, T1, T2, ldx):
    """efts_attn_soft_index: scores [B, T2, T1 + ldx] (the extra columns hold 7.0) -> soft index and masked alpha"""
    g, tl, ml = lengths(B, T1, T2, T1 * 1000 + T2 + 11)
    tm, mm = R.non_pad_mask(tl, T1), R.non_pad_mask(ml, T2)
    both = tm[:, :, None] & mm[:, None, :]
    scores = R.scores_for(tl, ml, T1, T2, g, ld=T1 + ldx)
    s32 = scores[:, :, :T1].contiguous()
    alpha = lambda t: R.attention_from_scores(t, tm).masked_fill(~both, 0.0)                    # noqa: E731
    sidx = lambda t: R.soft_index(alpha(t), R.index_vector(tm, t.dtype))                       # noqa: E731
    return dict(scores=scores, ld=T1 + ldx, tl=tl, ml=ml, tm=tm, mm=mm, refs=dict(soft_idx=_pair(sidx, s32), alpha=_pair(alpha, s32)))


def imv_case(T2):
    """efts_imv_scan on the ragged batch of 3: only item 0 can be non-zero (item 1 has one frame, item 2 one token)"""
    B = 3
    g, tl, ml = lengths(B, IMV_T1, T2, T2 + 23)
    mm = R.non_pad_mask(ml, T2)
    sidx = R.rising_soft_index(tl, ml, T2, g)
    return dict(B=B, sidx=sidx, tl=tl, ml=ml, mm=mm, refs=dict(imv=_pair(lambda t: R.imv_from_soft_index(t, mm, tl), sidx)))


def imv_hard_case(T2):
    """4 items: [0] decreases everywhere (every relu term 0: the 1e-8 clamp), [1] mel_len < T2 with a soft index that keeps rising
    beyond it (the mask comes before the maximum), [2] full length with a falling tail (a plateau: the maximum is not unique),
    [3] integers: rises by 8192 every third frame with a dip before each rise (partial sums up to 1.1e7 in the lanes, all exact)"""
    g = torch.Generator().manual_seed(T2 + 29)
    B = 4
    tl = torch.tensor([17, 31, 23, 40], dtype=torch.int32)
    ml = torch.tensor([T2, max(1, (2 * T2) // 3), T2, T2], dtype=torch.int32)
    mm = R.non_pad_mask(ml, T2)
    s = R.rising_soft_index(tl, ml, T2, g).double()
    j = torch.arange(T2, dtype=torch.float64)
    s[0] = 20.0 - 0.01 * j - 0.3 * torch.rand(T2, generator=g, dtype=torch.float64).cumsum(0)
    top = max(1, (3 * T2) // 4)
    s[2, top:] = s[2, top - 1] - 0.05 * (j[top:] - top + 1)
    s[3] = torch.where(j.long() % 3 == 2, -5.0, 1.0) * 1024.0 + torch.floor(j / 3) * 2048.0
    sidx = s.float()
    return dict(B=B, sidx=sidx, tl=tl, ml=ml, mm=mm, refs=dict(imv=_pair(lambda t: R.imv_from_soft_index(t, mm, tl), sidx)))


def _imv32(tl, ml, T2, g):
    """float32 IMV: the float64 IMV of a rising soft index, rounded"""
    return R.imv_from_soft_index(R.rising_soft_index(tl, ml, T2, g).double(), R.non_pad_mask(ml, T2), tl).float()


def epos_case(B, T1, T2):
    """efts_aligned_positions: IMV -> e, and the method-1 duration target the kernel can append"""
    g, tl, ml = lengths(B, T1, T2, T1 * 1000 + T2 + 12)
    tm, mm = R.non_pad_mask(tl, T1), R.non_pad_mask(ml, T2)
    imv = _imv32(tl, ml, T2, g)
    e = lambda t: R.aligned_positions(t, R.index_vector(tm, t.dtype), mm, tm, SIGMA_E)          # noqa: E731
    lde = lambda t: R.duration_target(e(t), tl, ml, OFFSET, True)                               # noqa: E731
    return dict(imv=imv, tl=tl, ml=ml, tm=tm, mm=mm, refs=dict(e=_pair(e, imv), lde=_pair(lde, imv)))


def dur_case(B, T1, method1):
    """efts_duration_target: positions that rise by positive steps to 0.9 * mel_len, so that both methods take the log of a number
    above the offset"""
    T2 = 8 * T1 + 3
    g, tl, ml = lengths(B, T1, T2, T1 * 1000 + 13)
    tm = R.non_pad_mask(tl, T1)
    u = (0.2 + torch.rand(B, T1, generator=g, dtype=torch.float64)) * tm
    e = (u.cumsum(1) / u.sum(1, keepdim=True) * 0.9 * ml.double()[:, None] * tm).float()
    return dict(e=e, tl=tl, ml=ml, tm=tm, T2=T2, refs=dict(lde=_pair(lambda t: R.duration_target(t, tl, ml, OFFSET, method1), e)))


def align_case(B, T1, T2, method1):
    """efts_imv_align: soft index -> IMV, e and the duration target of either method, each against the float64 composition"""
    g, tl, ml = lengths(B, T1, T2, T1 * 1000 + T2 + 14)
    tm, mm = R.non_pad_mask(tl, T1), R.non_pad_mask(ml, T2)
    sidx = R.rising_soft_index(tl, ml, T2, g)
    imv = lambda t: R.imv_from_soft_index(t, mm, tl)                                            # noqa: E731
    e = lambda t: R.aligned_positions(imv(t), R.index_vector(tm, t.dtype), mm, tm, SIGMA_E)     # noqa: E731
    lde = lambda t: R.duration_target(e(t), tl, ml, OFFSET, method1)                            # noqa: E731
    return dict(sidx=sidx, tl=tl, ml=ml, tm=tm, mm=mm, refs=dict(imv=_pair(imv, sidx), e=_pair(e, sidx), lde=_pair(lde, sidx)))


def align_exact_case():
    """A soft index of small integers: every difference, partial sum and the maximum (a power of two) of the scan is an exact
    float32 in any association, the quotient by a power of two is exact and the product with text_len - 1 is rounded once on both
    sides, so the kernel must give the float32 transcription bit for bit."""
    B, T1, T2 = 3, 37, 211
    g = torch.Generator().manual_seed(5)
    tl = torch.tensor([37, 20, 9], dtype=torch.int32)
    ml = torch.tensor([211, 150, 97], dtype=torch.int32)
    mm = R.non_pad_mask(ml, T2)
    step = torch.randint(-2, 2, (B, T2), generator=g)              # steps of -2 .. 1 between neighbouring frames
    for b in range(B):                                              # the last live step makes the relu-cumsum end on exactly 256
        last = int(ml[b]) - 1
        step[b, last] = 256 - int(torch.relu(step[b, 1:last]).sum())
    sidx = step.cumsum(1)
    sidx = sidx.float()
    imv32 = R.imv_from_soft_index(sidx, mm, tl)
    pi = (torch.relu(sidx[:, 1:] - sidx[:, :-1]).cumsum(1) * mm[:, 1:])
    assert float(pi.max(1).values.min()) == 256.0 and float(pi.max()) == 256.0
    return dict(B=B, T1=T1, T2=T2, sidx=sidx, tl=tl, ml=ml, imv32=imv32)


def ralpha_case(B, T1, T2, masked):
    """efts_reconst_alpha.  Masked (training) form: ragged lengths, e of the float64 stages, alpha' zero outside text x mel.
    Inference form: the kernel gets no lengths and every (i, j) is live, so the items span T1 x T2 as inference batches of one do."""
    g, tl, ml = lengths(B, T1, T2, T1 * 1000 + T2 + 15)
    if not masked:
        tl, ml = torch.full_like(tl, T1), torch.full_like(ml, T2)
    tm, mm = R.non_pad_mask(tl, T1), R.non_pad_mask(ml, T2)
    e = R.aligned_positions(_imv32(tl, ml, T2, g).double(), R.index_vector(tm, torch.float64), mm, tm, SIGMA_E).float()
    if masked:
        fn = lambda t: R.masked_ralpha(t, SIGMA, mm, tm)                                        # noqa: E731
    else:
        ones1, ones2 = torch.ones(B, T1, dtype=torch.bool), torch.ones(B, T2, dtype=torch.bool)
        fn = lambda t: R.reconstruct_alignment(t, SIGMA, ones2, ones1)                          # noqa: E731
    return dict(e=e, tl=tl, ml=ml, tm=tm, mm=mm, refs=dict(ralpha=_pair(fn, e)))


def chain_case(B, T1, T2):
    """scores -> alpha' through the whole forward block (the lengths and scores of the backward chain test)"""
    g = torch.Generator().manual_seed(T1 * 1000 + T2 + 3)
    tl, ml = R.ragged_lengths(B, T1, g), R.ragged_lengths(B, T2, g)
    scores = R.scores_for(tl, ml, T1, T2, g)
    blk64, blk32 = R.alignment_block(scores.double(), tl, ml, SIGMA, SIGMA_E), R.alignment_block(scores, tl, ml, SIGMA, SIGMA_E)
    refs = {k: (blk64[k], blk32[k]) for k in ("soft_idx", "imv", "e", "ralpha")}
    return dict(scores=scores, tl=tl, ml=ml, tm=blk64["text_mask"], mm=blk64["mel_mask"], refs=refs)


# =====================================================================================================================
# activations
# =====================================================================================================================
ACT_EXTRA = [("ELU", {}), ("CELU", {}), ("Softplus", {}), ("Hardtanh", {})]            # the modules' defaults, next to ACTS of test_gpu_variants.py
ACT_SHAPES = [(1, 4), (63, 124), (64, 128), (65, 132), (130, 512)]
RANDOM_SHAPE = (65, 132)
TAILS = (12.0, 19.5, 20.5, 30.0, 60.0, 88.0)
BANDS = (("|z|<=1", 0.0, 1.0), ("1<|z|<=8", 1.0, 8.0), ("|z|>8", 8.0, float("inf")))
# f' = 1 - t^2 (Tanh) and s (1 - s) (Sigmoid) beyond |z| = 8 are below the float32 resolution of t and s next to 1 (tanh'(8.02) =
# 4.3e-7, one ulp of t is 6e-8): measured against the band's own maximum the float32 transcription itself is off by 0.3 and 5e-3, and
# no input moves that.  These two gradients are therefore measured in two bands, the outer one being |z| > 1: every grid point is
# still compared, against the scale of f' where float32 resolves it.
GRAD_BANDS_SATURATING = (BANDS[0], ("|z|>1", 1.0, float("inf")))


def act_list():
    from test_gpu_variants import ACTS
    return [(n, {k: v for k, v in p.items() if k != "inplace"}) for n, p in ACTS] + ACT_EXTRA


def act_id(name, params):
    return name + "".join(f"_{k}{v}" for k, v in params.items())


def act_breakpoints(name, params):
    if name in ("ReLU", "LeakyReLU", "ELU", "CELU", "SELU"):
        return [0.0]
    if name in ("Hardswish", "Hardsigmoid"):
        return [-3.0, 3.0]
    if name == "Hardtanh":
        return [params.get("min_val", -1.0), params.get("max_val", 1.0)]
    if name == "ReLU6":
        return [0.0, 6.0]
    if name == "Softplus":
        return [params.get("threshold", 20.0) / params.get("beta", 1.0)]
    if name == "Mish":
        return [20.0]
    return []


def act_grid(name, params):
    """float32: 512 points (k + 1/2) / 32 in (-8, 8) (no multiple of 1/32, so none on a breakpoint), the tails, +-0 and both sides of
    every breakpoint at 2^-10"""
    dense = (torch.arange(-256, 256, dtype=torch.float64) + 0.5) / 32.0
    tails = torch.tensor([s * t for t in TAILS for s in (1.0, -1.0)], dtype=torch.float64)
    bp = torch.tensor(act_breakpoints(name, params), dtype=torch.float32).double()       # the breakpoint as float32 holds it
    near = torch.cat([bp - 2.0 ** -10, bp + 2.0 ** -10])
    z = torch.cat([dense, tails, torch.tensor([0.0, -0.0], dtype=torch.float64), near]).float()
    for b in bp.tolist():
        if b != 0.0:
            assert not bool((z.double() == b).any())
    return z


def act_bands(name, which):
    return GRAD_BANDS_SATURATING if which == "grad" and name in ("Tanh", "Sigmoid") else BANDS


def act_case(name, params, rows, c, kind="grid"):
    """z [rows, c] (the grid tiled in a fixed stride, or 3 * randn), residual, 0/1 row mask and upstream gradient; f and f' of torch's own module in float64
    and float32"""
    g = torch.Generator().manual_seed(rows * 1000 + c)
    n = rows * c
    if kind == "grid":
        grid = act_grid(name, params)
        # element k takes grid point (300 + 131 k) mod len: a walk through the whole grid that spreads even 4 elements over the range
        z = grid[(300 + 131 * torch.arange(n)) % len(grid)].reshape(rows, c).contiguous()
        assert n < len(grid) or len(torch.unique(z.view(torch.int32))) == len(grid)
    else:
        z = 3.0 * torch.randn(rows, c, generator=g)
    resid = torch.randn(rows, c, generator=g)
    up = torch.randn(rows, c, generator=g)
    rm = (torch.rand(rows, generator=g) > 0.3).float()
    if rows > 1:
        rm[0], rm[rows - 1] = 1.0, 0.0
    db0 = torch.randn(c + 4, generator=g)                                              # what dbias holds before the kernel adds to it, and 4 guard floats
    mod = getattr(torch.nn, name)(**params)

    def f_df(dtype):
        x = z.to(dtype).requires_grad_(True)
        y = mod(x)
        (d,) = torch.autograd.grad(y.sum(), x)
        return y.detach(), d

    (f64, d64), (f32, d32) = f_df(torch.float64), f_df(torch.float32)
    return dict(z=z, resid=resid, up=up, rm=rm, db0=db0, f=(f64, f32), df=(d64, d32))


def act_apply_refs(cs, use_resid, use_mask):
    """y = (resid + f(z)) * rowmask in float64 and float32"""
    out = []
    for f, dt in zip(cs["f"], (torch.float64, torch.float32)):
        y = f + cs["resid"].to(dt) if use_resid else f
        out.append(y * cs["rm"].to(dt)[:, None] if use_mask else y)
    return tuple(out)


def act_grad_refs(cs, use_mask):
    """dZ = G * rowmask * f'(z) in float64 and float32"""
    out = []
    for d, dt in zip(cs["df"], (torch.float64, torch.float32)):
        gm = cs["up"].to(dt) * cs["rm"].to(dt)[:, None] if use_mask else cs["up"].to(dt)
        out.append(gm * d)
    return tuple(out)


def act_dbias_refs(cs, use_mask):
    """dbias + column sums of dZ in float64 and float32"""
    c = cs["z"].shape[1]
    d64, d32 = act_grad_refs(cs, use_mask)
    return cs["db0"][:c].double() + d64.sum(0), cs["db0"][:c] + d32.sum(0)


def band_masks(z, bands):
    a = z.abs()
    return [(label, (a > lo) & (a <= hi) if lo > 0 else a <= hi) for label, lo, hi in bands]
