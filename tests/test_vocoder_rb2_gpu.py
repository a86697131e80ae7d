"""GPU (-m gpu): HiFi-GAN generators built from ResBlock2 (`resblock: "2"`, the V3 family) and the fused launch `efts_resblock2`
(csrc/efts_resblock2.hip) against tests/vocoder_rb2_reference.py.

Configurations (tests/vocoder_rb2_reference.py:CASES; lengths in mel frames):
    v3-small   the V3 configuration, lengths 5 / 3 at T = 5: 128 / 64 / 32 channels (4, 2, 1 column blocks), the 72-row window span of
               k = 7, d = 12 that two efts_gemm launches cannot run, 5 gap frames; item 1 sits exactly one minimum gap behind item 0
    narrow     32 -> 16, 8 channels (less than one operand chunk), rates (4, 2), kernels (3, 11) with dilations (1, 3) / (1, 5), 20 mels,
               lengths 9 / 1 / 14: a one-frame item
    limit      64 -> 32, 16, rates (4, 4), one kernel 9 with dilations (4, 12): halo sum exactly 64, second span 96; 13 / 13 at T = 13
    tiles      the narrow configuration, one item of 90 frames: 720 rows at the last stage = 3.87 row tiles of 186 (k = 3) and 5.07 of
               142 (k = 11): a partial last tile behind more than three full ones
and the kernel alone through ctypes: (rows, c, k, d0, d1) = (700, 128, 7, 3, 12), (300, 64, 5, 2, 6), (333, 32, 3, 1, 2), (257, 16, 11, 1, 5),
(200, 8, 9, 4, 12) and (150, 96, 3, 1, 1) -- the three-column-block instantiation no generator case reaches -- with ldx, ldo > c, rows of
the mask zero inside the space, the output prefilled with 7.0, the input plane written by its producer (efts_act_bwd mode 3) and the
float64 reference computed from the plane and the packed weights as the kernel reads them (decoded hi + lo).

Bounds (none of them new).  precision "fp32": `kernel_check._check`, max(8 * e32, 2e-6) with 8 * e32 <= 2e-4 asserted.  "bf16x3" /
"bf16": a ResBlock2 is two contractions with a plane between them, the shape of `res_pair` in tests/test_vocoder_stages_gpu.py, and is
held to its rule: 2 x 2e-5 / 2 x 2e-2 of max |ref|, plus the plane resolution (2^-16 / 2^-8) where the input was decoded from a plane
(the kernel alone).  Asserted with ==: rows past an item's length, between items, the guard rows and the padding columns of every block
output, the final audio past every length, and what lies outside [m][c] of the kernel's output (still 7.0).
Both arms (`fused_resblock2` True / False) are held to the same bound wherever both can run; `forward(mel, lengths)` is `torch.equal`
to the items alone and a hipGraph replay to the eager run.  Whole generator: fp32 against float64 with `_check(chain=True)`; the golden
of the reference Generator (tests/golden/hifigan_rb2_small.npz) with the tolerances of tests/test_vocoder.py (bf16x3 1e-3, bf16 6e-2;
fp32 held to the bf16x3 figure).

Measured on one MI355X (worst over all cases of a kind; fp32: err / e32 where 8 * e32 is the bound; bf16x3 / bf16: err (bound)):

    kind                  checks per precision  fp32: worst err / e32                          bf16x3                              bf16
    efts_resblock2 alone   6                    2.47 (700x128 k=7 d=(3,12): 6.2e-07 / 2.5e-07)  3.1e-06 (5.5e-05) 150x96 k=3        1.1e-03 (4.4e-02) 150x96 k=3
    resblock2.fused       24                    2.90 (v3-small r0.1: 8.3e-07 / 2.9e-07)         4.7e-06 (4.0e-05) tiles r0.0        2.3e-03 (4.0e-02) tiles r1.1
    resblock2.composed    14                    2.90 (v3-small r0.1: 8.3e-07 / 2.9e-07)         4.7e-06 (4.0e-05) tiles r0.0        2.3e-03 (4.0e-02) tiles r1.1
    golden (max abs)       1                    6.6e-07                                         9.9e-06 (1e-3)                      5.7e-03 (6e-2)
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vocoder_rb2_reference as RR
from kernel_check import _call, _check, _dev, _rel, _st, load_lib, unpack_plane

pytestmark = pytest.mark.gpu

SPLIT = {"bf16": 1, "bf16x3": 2, "fp32": 3}
LAUNCH = {"bf16x3": 2e-5, "bf16": 2e-2}                   # one contraction launch, of max |ref| (tests/test_vocoder_stages_gpu.py)
RESOLUTION = {"fp32": 0.0, "bf16x3": 2.0 ** -16, "bf16": 2.0 ** -8}
PRECISIONS = ["fp32", "bf16x3", "bf16"]
GOLD = os.path.join(os.path.dirname(__file__), "golden", "hifigan_rb2_small.npz")
GOLD_TOL = {"fp32": 1e-3, "bf16x3": 1e-3, "bf16": 6e-2}   # tests/test_vocoder.py::test_generator_matches_reference_golden


@pytest.fixture(scope="module")
def lib():
    return load_lib()


@functools.lru_cache(maxsize=None)
def _case(name):
    cs = RR.CASES[name]
    P = RR.fill(cs["cfg"], cs["seed"])
    mel = RR.mel_input(cs["cfg"], len(cs["lengths"]), cs["T"], cs["seed"])
    return cs, P, mel, RR.Reference(cs["cfg"], P, torch.float64), RR.Reference(cs["cfg"], P, torch.float32)


@functools.lru_cache(maxsize=None)
def _whole(name):
    cs, P, mel, R64, R32 = _case(name)
    return R64.forward(mel, cs["lengths"])["out"], R32.forward(mel, cs["lengths"])["out"]


def _model(name, precision, graphs=False, fused=True):
    from efficient_tts_amd.vocoder import HiFiGANGenerator
    cs, P, _, _, _ = _case(name)
    m = HiFiGANGenerator(cs["cfg"], precision=precision)
    m.load_state_dict(P)
    m = m.to(_dev()).eval()
    m.graphs, m.fused_resblock2 = graphs, fused
    return m


def _items(full, c, rate, pitch, lens, guard, zeros=True):
    """the items of a row space [alloc][>= c] as [1, c, len * rate] each; with `zeros`, everything that is not a live row and column of
    an item must be exactly 0"""
    full = full.cpu()
    live = torch.zeros(full.shape[0], dtype=torch.bool)
    items = []
    for b, n in enumerate(lens):
        lo = guard + b * pitch * rate
        live[lo:lo + n * rate] = True
        items.append(full[lo:lo + n * rate, :c].t().contiguous()[None].float())
    if zeros:
        assert bool((full[~live] == 0).all()), "rows outside the items must be exactly 0"
        assert bool((full[:, c:] == 0).all()), "padding columns must be exactly 0"
    return items


def _bounded(prec, kind, case, got, ref64, ref32, from_plane):
    """two contraction launches' worth (the res_pair rule), or `_check` in fp32 mode"""
    if prec == "fp32":
        _check(kind, f"{case} {prec}", got, ref64, ref32)
        return
    assert bool(torch.isfinite(got).all())
    err, bound = _rel(got.double(), ref64), 2 * LAUNCH[prec] + (RESOLUTION[prec] if from_plane else 0.0)
    print(f"RATIO {kind} {case} {prec} err={err:.3e} bound={bound:.3e} ratio={err / bound:.2f}")
    assert err <= bound, f"{kind} {case} {prec}: error {err:.3e} vs float64, bound {bound:.3e}"


# =====================================================================================================================
# the kernel alone
# =====================================================================================================================
ALONE = [(700, 128, 7, 3, 12), (300, 64, 5, 2, 6), (333, 32, 3, 1, 2), (257, 16, 11, 1, 5), (200, 8, 9, 4, 12), (150, 96, 3, 1, 1)]


def _conv_rows(p, w, b, k, d):
    """rows [m][c] (already activated) convolved along the rows: [m][c]"""
    y = F.conv1d(p.t()[None], w, b, padding=(k - 1) // 2 * d, dilation=d)
    return y[0].t()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("m,c,k,d0,d1", ALONE)
def test_kernel_alone_vs_fp64(lib, m, c, k, d0, d1, precision):
    from efficient_tts_amd import lib as L
    from efficient_tts_amd.ops import PackedWeight, Plane
    dev, sp, slope = _dev(), SPLIT[precision], 0.1
    g = torch.Generator().manual_seed(m * 131 + c * 7 + k)
    ldx, ldo, guard = c + 4, c + 8, 64
    x = torch.randn(m, ldx, generator=g)
    mask = torch.ones(m)
    mask[m // 3:m // 3 + 7] = 0                                      # zero rows inside the space
    mask[m - 5:m - 3] = 0
    mask[0] = 0
    w = [torch.randn(c, c, k, generator=g) / (c * k) ** 0.5 for _ in range(2)]
    b = [0.1 * torch.randn(c, generator=g) for _ in range(2)]
    xd, md = x.to(dev), mask.to(dev)
    # the input plane as its producer writes it: leaky(x) * mask (efts_act_bwd mode 3, HiFiGANGenerator._stage_upsample)
    p0 = Plane(guard + m + 8, c, sp, dev, guard_lo=guard)
    xc = xd[:, :c].contiguous()
    _call("efts_act_bwd", lib.efts_act_bwd(xc.data_ptr(), xc.data_ptr(), None, md.data_ptr(), slope, 3, None, p0.ptr, p0.ld, sp, None, m, c, _st()))
    pw = []
    for t in range(2):
        pw.append(PackedWeight(c, c, k, sp, dev))
        pw[-1].pack(w[t].to(dev).contiguous())
    bd = [v.to(dev) for v in b]
    out = torch.full((m + 3, ldo), 7.0, device=dev)
    a = L.ResBlock2Args()
    a.x, a.ldx, a.p0, a.ldp = xd.data_ptr(), ldx, p0.ptr, p0.ld
    a.w0, a.w1, a.ldw, a.w_tap_stride = pw[0].ptr, pw[1].ptr, pw[0].ld, pw[0].tap_stride
    a.bias0, a.bias1, a.rowmask, a.out, a.ldo = bd[0].data_ptr(), bd[1].data_ptr(), md.data_ptr(), out.data_ptr(), ldo
    a.split, a.m, a.c, a.k, a.d0, a.d1, a.slope = sp, m, c, k, d0, d1, slope
    _call("efts_resblock2", lib.efts_resblock2(ctypes.byref(a), _st()))
    torch.cuda.synchronize()
    out = out.cpu()
    # the reference on the device's own operands, decoded as the kernel reads them
    kp = p0.nchunk * (64 if sp == 1 else 32)
    pdec = unpack_plane(p0.buf, 1, p0.buf.shape[0], p0.buf.shape[0], kp, sp)[0][guard:guard + m, :c]
    wdec = [unpack_plane(q.buf.view(k * c, q.ld), 1, k * c, k * c, kp, sp)[0].view(k, c, kp)[:, :, :c].permute(1, 2, 0).contiguous() for q in pw]

    def ref(dt):
        xx, mm = x[:, :c].to(dt), mask.to(dt)[:, None]
        y1 = (xx + _conv_rows(pdec.to(dt), wdec[0].to(dt), b[0].to(dt), k, d0)) * mm
        return (y1 + _conv_rows(F.leaky_relu(y1, slope), wdec[1].to(dt), b[1].to(dt), k, d1)) * mm
    got = out[:m, :c]
    _bounded(precision, "efts_resblock2", f"{m}x{c} k={k} d=({d0},{d1})", got, ref(torch.float64), ref(torch.float32), True)
    assert bool((out[m:] == 7.0).all()) and bool((out[:, c:] == 7.0).all())           # untouched
    assert bool((got[mask == 0] == 0).all())                                          # masked rows are exactly 0


# =====================================================================================================================
# every block of a generator, both arms
# =====================================================================================================================
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(RR.CASES))
def test_every_block_vs_fp64(lib, name, precision, fused):
    from efficient_tts_amd.vocoder import _GUARD
    cs, P, mel, R64, R32 = _case(name)
    cfg, lens, T = cs["cfg"], cs["lengths"], cs["T"]
    m = _model(name, precision, fused=fused)
    keep = {}
    audio = m(mel.to(_dev()), torch.tensor(lens), keep=keep)
    torch.cuda.synchronize()
    keep = {k: v.cpu() if torch.is_tensor(v) else v for k, v in keep.items()}
    pitch = keep["pitch"]
    assert pitch == T + m.gap_frames
    rate = 1
    for i, u in enumerate(R64.rates):
        rate *= u
        c = RR.VR.channels(cfg, i)
        up = _items(keep[f"up{i}"], c, rate, pitch, lens, 0, zeros=False)
        for j in range(len(R64.res_kernels)):
            n = R64.block(i, j)
            ran_fused = m._rb2_fused(c, R64.res_kernels[j], tuple(R64.res_dilations[j]))
            got = _items(keep[f"r{i}.{j}"], c, rate, pitch, lens, _GUARD)
            ref64, ref32 = [R64.res_block(n, x) for x in up], [R32.res_block(n, x) for x in up]
            _bounded(precision, "resblock2.fused" if ran_fused else "resblock2.composed", f"{name}:r{i}.{j}",
                     torch.cat(got, 2), torch.cat(ref64, 2), torch.cat(ref32, 2), False)
    audio = audio.cpu()
    assert audio.shape == (len(lens), 1, T * rate)
    out = _items(keep["out"], 1, rate, pitch, lens, 0)
    for b, n in enumerate(lens):
        assert torch.equal(audio[b, :, :n * rate], out[b][0]) and bool((audio[b, :, n * rate:] == 0).all())
    if precision == "fp32":
        w64, w32 = _whole(name)
        _check("generator", f"{name} fp32 fused={fused}", audio, w64, w32, chain=True)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ["v3-small", "limit"])
def test_batch_equals_items_alone_and_graph_replay_equals_eager(name, precision):
    """item 1 of both cases begins exactly one minimum gap behind item 0's last row: its blocks must not see item 0.
    The launches are captured as forward() captures them: the graph cache runs the first two calls of a shape eagerly and then decides
    by the host's share of the time, so the policy is pinned to "graph" here and the capture is asserted (`captures`).  A replay gives
    the bits of the eager run in both arms, and `fused_resblock2` is part of the graph tag: flipping it captures again."""
    cs, P, mel, _, _ = _case(name)
    lens, T = cs["lengths"], cs["T"]
    hop = int(np.prod(cs["cfg"]["upsample_rates"]))
    x, l = mel.to(_dev()), torch.tensor(lens)
    eager = {}
    for fused in (True, False):
        e = _model(name, precision, graphs=False, fused=fused)
        eager[fused] = e(x, l).clone()
    m = _model(name, precision, graphs=True, fused=True)
    cache = m._graph_cache
    cache.EAGER_MAX_HOST_SHARE = -1.0                       # the third call of a shape captures whatever the second one's timing says
    ys = [m(x, l).clone() for _ in range(4)]                # eager, eager (timed), capture + replay, replay
    assert cache.captures == 1 and cache.entries[("voc", len(lens), T)].graph is not None
    for y in ys:
        assert torch.equal(y, eager[True]), precision
    m.fused_resblock2 = False                               # another tag: the graph is dropped, a timed eager call, then a new capture
    zs = [m(x, l).clone() for _ in range(3)]
    assert cache.captures == 2 and cache.entries[("voc", len(lens), T)].graph is not None
    for z in zs:
        assert torch.equal(z, eager[False]), precision
    # (the arms may agree to the bit -- the fused launch keeps efts_gemm's summation order -- so the re-capture is shown by the counter)
    m.fused_resblock2 = True
    y = m(x, l).clone()
    y = m(x, l).clone()
    assert cache.captures == 3 and torch.equal(y, eager[True])
    for b, n in enumerate(lens):                            # each item alone, through three calls so that the last one is a replay too
        xb = mel[b:b + 1, :, :n].contiguous().to(_dev())
        for _ in range(3):
            alone = m(xb).clone()
        assert torch.equal(y[b, :, :n * hop], alone[0]), (precision, b)
        assert bool((y[b, :, n * hop:] == 0).all())
    assert cache.captures == 3 + len({n for n in lens})     # one graph per distinct alone shape (B = 1, T = n)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_generator_matches_reference_golden(precision):
    from efficient_tts_amd.vocoder import HiFiGANGenerator
    g = np.load(GOLD)
    m = HiFiGANGenerator(RR.GOLDEN, precision=precision)
    m.load_state_dict({k: torch.from_numpy(g[k]) for k in g.files if k not in ("mel", "audio")})
    m = m.to(_dev()).eval()
    y = m(torch.from_numpy(g["mel"]).to(_dev()))
    assert y.shape == g["audio"].shape
    err = float(np.abs(y.cpu().numpy() - g["audio"]).max())
    print(precision, "max abs err vs the reference Generator", err)
    assert err <= GOLD_TOL[precision], (precision, err)
    m.remove_weight_norm()
    assert float((m(torch.from_numpy(g["mel"]).to(_dev())) - y).abs().max()) <= 1e-5
