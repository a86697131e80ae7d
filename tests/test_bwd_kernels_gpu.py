"""GPU (-m gpu): every training-side pointwise / reduction kernel alone against a float64 reference of the same operation.

The exports below are called with torch tensors as buffers through their wrappers in `efficient_tts_amd.ops`, the way
efficient_tts_amd/train.py does (the forward-side ones, and the refusal cases, directly through `efficient_tts_amd.lib`) -- no model,
no TrainEngine, no golden file:

    efts_alpha_bwd  efts_e_bwd  efts_imv_bwd  efts_attn_bwd  efts_embed_bwd  efts_loss_bwd  efts_masked_losses
    efts_layernorm_rows  efts_layernorm_dot  efts_layernorm_bwd  efts_cumsum_rows  efts_sumsq  efts_scale_unless_one

Reference.  torch autograd in float64 on the CPU through tests/bwd_reference.py (plain transcriptions of the oracle functions,
pinned to the oracle by tests/test_bwd_reference_cpu.py), or the closed-form float64 value for the reductions.  Kernel and
reference get the SAME float32 inputs (the reference upcasts them), so the sign of a difference of two inputs -- every
relu(s_j - s_{j-1}) decision -- is the same on both sides.  A kernel's stage inputs (alpha', e, pi, the soft index) are computed in
float64 from its primary input and rounded to float32; the upstream gradient is random.

Metric and bound.  `_rel` = max |got - ref| / max |ref| over the tensor.  For every case the same transcription is also evaluated
in float32 torch on the CPU; its error against float64 is `e32`, and the kernel must be within max(8 * e32, 2e-6).  The bound can
not grow until it hides an error: 8 * e32 <= 2e-4 is asserted for every case (inputs as the model produces them: a soft index that
rises from 0 to text_len - 1 with noise of about 0.3, standard-normal upstream gradients, sigma 0.01, sigma_e 0.5).  Values that
must be exactly zero or bit-identical are asserted with ==.

What each kernel takes from its caller (efficient_tts_amd/train.py, TrainEngine.forward_backward):
  * efts_alpha_bwd reads alpha' as the forward masked it (0 outside text x mel), so padded frames and padded tokens drop out of
    r and de whatever dalpha holds there, as long as it is finite; the caller's dalpha = V . dH^T is 0 at frames j >= mel_len
    because dH is masked (train.py, `dH = self._stack_bwd(... len2 ...)` feeding the `dAp` product).  The tests build dalpha
    that way and leave random finite numbers in the padded token rows.
  * efts_e_bwd and efts_imv_bwd loop over i < text_len and j < mel_len themselves: they need nothing zeroed.
  * efts_attn_bwd writes rows (b, j < T2) of the plane only; the gap rows j >= T2 of the row space are the caller's (zero-filled
    once by ops.Plane).  Checked here by filling the buffer with 0xAB first.
  * efts_layernorm_bwd in its `ddur * w` form does not mask dy: ddur must be 0 on padded tokens and gap rows, which efts_loss_bwd
    guarantees (train.py, the `efts_loss_bwd` call writes `Bddur`, 0 at i >= text_len and in the gap rows).

Measured on one MI355X: the worst `kernel error / e32` of each kernel over its cases whose bound is the 8 * e32 branch
(e32 > 2.5e-7), and the worst absolute error where the 2e-6 floor is the bound.

    kernel                     cases  worst err / e32 (e32 > 2.5e-7)                     worst err under the 2e-6 floor
    efts_alpha_bwd.r               9  -                                                  7.2e-08  (3x5x64)
    efts_alpha_bwd.de              9  0.17  (3x9x1500: 1.6e-07 / 9.7e-07)                1.6e-07  (2x128x800)
    efts_e_bwd                     8  0.76  (3x9x128: 2.4e-07 / 3.1e-07)                 0.0e+00  (3x1x33)
    efts_imv_bwd                  29  0.97  (T2=800[item 1]: 3.1e-07 / 3.2e-07)          6.6e-07  (T2=4100[item 1])
    efts_attn_bwd                  7  0.30  (3x37x211: 1.0e-06 / 3.4e-06)                0.0e+00  (3x1x33)
    chain                          3  0.40  (chain 3x37x211: 2.1e-06 / 5.3e-06)          -
    efts_embed_bwd                 2  -                                                  8.3e-08  (c=512)
    efts_loss_bwd.dmel             6  -                                                  6.7e-08  (ldm=96 gscale=None)
    efts_loss_bwd.ddur             6  -                                                  3.0e-08  (ldm=96 gscale=None)
    efts_masked_losses.loss        3  -                                                  6.3e-08  (ldm=96)
    efts_masked_losses.mel         3  -                                                  1.6e-08  (ldm=96)
    efts_masked_losses.dur         3  -                                                  3.8e-08  (ldm=96)
    efts_layernorm_rows           14  -                                                  1.4e-07  (8x512)
    efts_layernorm_dot            14  0.34  (8x2048: 1.1e-07 / 3.1e-07)                  1.5e-07  (9x256)
    efts_layernorm_bwd.dz         42  -                                                  2.0e-07  (ddur 9x2048)
    efts_layernorm_bwd.dgamma     42  2.18  (ddur 4100x2048: 5.7e-07 / 2.6e-07)          8.9e-07  (dy 4100x2048)
    efts_layernorm_bwd.dbeta      42  2.97  (dy 4100x512: 8.2e-07 / 2.8e-07)             7.6e-07  (ddur_rowmask 4100x2048)
    efts_layernorm_bwd.dbias      42  -                                                  7.7e-07  (ddur_rowmask 4100x2048)
    efts_layernorm_bwd.dw         28  0.50  (ddur_rowmask 4100x2048: 8.1e-07 / 1.6e-06)  2.1e-07  (ddur_rowmask 9x256)
    efts_layernorm_bwd.db         28  -                                                  7.5e-07  (ddur_rowmask 4100x2048)
    efts_cumsum_rows               7  -                                                  1.8e-07  (T=1000)
    efts_sumsq                     6  -                                                  8.2e-08  (n=1048577)
    largest e32 of a single-stage case: 2.2e-05

Every ratio is below 8 (the largest, 3.0, is the order of the 513 atomic adds per column in efts_layernorm_bwd's dbeta); no factor was widened.
`chain` is test_alignment_backward_chain_vs_fp64, whose bound is capped at 2e-4 instead (its docstring says why).
"""
from types import SimpleNamespace

import pytest
import torch

import bwd_reference as R
from efficient_tts_amd import ops as O
from kernel_check import COND, FACTOR, FLOOR, _call, _check, _dev, _rel, _st, load_lib   # noqa: F401  (the metric and the bound: tests/kernel_check.py)

pytestmark = pytest.mark.gpu

SIGMA, SIGMA_E = 0.01, 0.5


@pytest.fixture(scope="module")
def lib():
    return load_lib()


def _grad(fn, x32, up32, dtype):
    """d <fn(x), up> / dx with everything in `dtype`"""
    x = x32.to(dtype).requires_grad_(True)
    (g,) = torch.autograd.grad((fn(x) * up32.to(dtype)).sum(), x)
    return g


def _lengths(B, T1, T2, seed):
    """ragged; item 0 spans both padded lengths, the last item has text_len 1 and (B >= 3) item 1 has mel_len 1"""
    g = torch.Generator().manual_seed(seed)
    tl = R.ragged_lengths(B, T1, g, last=1)
    ml = R.ragged_lengths(B, T2, g)
    if B >= 3:
        ml[1] = 1
    return g, tl, ml


def _stages(tl, ml, T1, T2, g):
    """float32 soft index and the float32-rounded float64 stages behind it"""
    tm, mm = R.non_pad_mask(tl, T1), R.non_pad_mask(ml, T2)
    sidx = R.rising_soft_index(tl, ml, T2, g)
    p64 = R.index_vector(tm, torch.float64)
    imv = R.imv_from_soft_index(sidx.double(), mm, tl).float()
    e = R.aligned_positions(imv.double(), p64, mm, tm, SIGMA_E).float()
    ralpha = R.masked_ralpha(e.double(), SIGMA, mm, tm).float()
    return tm, mm, sidx, imv, e, ralpha


def _upstream_dalpha(B, T1, T2, mm, g):
    """d alpha' as the caller's product with the masked dH leaves it: 0 at frames j >= mel_len, anything finite elsewhere"""
    return torch.randn(B, T1, T2, generator=g) * mm[:, None, :]


# =====================================================================================================================
# alignment block
# =====================================================================================================================
def _run_alpha_bwd(lib, ralpha, dA, e, tl, ml, B, T1, T2):
    dev = _dev()
    r = torch.full((B, T2), 7.0, device=dev)
    de = torch.full((B, T1), 7.0, device=dev)
    O.alpha_bwd(ralpha, dA, e, tl, ml, SIGMA, r, de, B, T1, T2)
    return r, de


@pytest.mark.parametrize("B,T1,T2", [(3, 1, 33), (3, 5, 64), (4, 9, 33), (3, 37, 211), (4, 100, 800), (2, 128, 800), (2, 203, 1500),
                                     (3, 203, 64), (3, 9, 1500)])
def test_alpha_bwd_vs_fp64(lib, B, T1, T2):
    """efts_alpha_bwd: r[b][j] = sum_i alpha'_ij dA_ij and de = d <alpha'(e), dA> / de through reconstruct_alignment.
    T1 mod 8 = 1, 5, 1, 5, 4, 0, 3: each of the r kernel's 4 waves meets the unrolled pair, the single-row tail, or gets no row at all."""
    dev = _dev()
    g, tl, ml = _lengths(B, T1, T2, T1 * 1000 + T2)
    tm, mm, _, _, e, ralpha = _stages(tl, ml, T1, T2, g)
    dA = _upstream_dalpha(B, T1, T2, mm, g)
    r, de = _run_alpha_bwd(lib, ralpha.to(dev), dA.to(dev), e.to(dev), tl.to(dev), ml.to(dev), B, T1, T2)
    torch.cuda.synchronize()
    case = f"{B}x{T1}x{T2}"
    _check("efts_alpha_bwd.r", case, r, (ralpha.double() * dA.double()).sum(1), (ralpha * dA).sum(1))
    fn = lambda t: R.masked_ralpha(t, SIGMA, mm, tm)                              # noqa: E731
    _check("efts_alpha_bwd.de", case, de, _grad(fn, e, dA, torch.float64), _grad(fn, e, dA, torch.float32))
    de = de.cpu()
    assert bool((de[~tm] == 0).all())                                             # padded tokens: exactly 0
    assert bool((r.cpu()[~mm] == 0).all())


def _run_e_bwd(lib, imv, e, de, tl, ml, B, T1, T2):
    dev = _dev()
    ws = torch.empty(2 * B * T1, device=dev)
    dpi = torch.full((B, T2), 7.0, device=dev)
    O.e_bwd(imv, e, de, tl, ml, SIGMA_E, ws, dpi, B, T1, T2)
    return dpi


@pytest.mark.parametrize("B,T1,T2", [(3, 37, 83), (3, 9, 128), (3, 100, 129), (2, 128, 256), (2, 203, 211), (2, 256, 1363), (3, 1, 33)])
def test_e_bwd_vs_fp64(lib, B, T1, T2):
    """efts_e_bwd: dpi = d <e(pi), de> / dpi through aligned_positions.  128-thread blocks over T2: T2 mod 128 = 83, 0, 1, 0, 83, 83
    and T2 < 128; T1 up to 256, the training limit of efts_expand."""
    dev = _dev()
    g, tl, ml = _lengths(B, T1, T2, T1 * 1000 + T2 + 1)
    tm, mm, _, imv, e, _ = _stages(tl, ml, T1, T2, g)
    de = torch.randn(B, T1, generator=g)
    dpi = _run_e_bwd(lib, imv.to(dev), e.to(dev), de.to(dev), tl.to(dev), ml.to(dev), B, T1, T2)
    torch.cuda.synchronize()
    fn = lambda t: R.aligned_positions(t, R.index_vector(tm, t.dtype), mm, tm, SIGMA_E)      # noqa: E731
    _check("efts_e_bwd", f"{B}x{T1}x{T2}", dpi, _grad(fn, imv, de, torch.float64), _grad(fn, imv, de, torch.float32))
    assert bool((dpi.cpu()[~mm] == 0).all())                                      # padded frames: exactly 0


def test_e_bwd_at_its_lds_limit(lib):
    """A text padded to T1 = 4096, the largest whose 4 * T1 floats fit the launch (64 KiB): it runs, and gives the float64 gradient
    (text lengths 128 and 70 inside the padding, so that the inputs are conditioned like the other cases');
    4097 is refused with a message (tests/test_bwd_reference_cpu.py checks the refusal without a device)."""
    dev = _dev()
    B, T1, T2 = 2, 4096, 192
    g = torch.Generator().manual_seed(4096)
    tl, ml = torch.tensor([128, 70], dtype=torch.int32), torch.tensor([T2, 150], dtype=torch.int32)
    tm, mm, _, imv, e, _ = _stages(tl, ml, T1, T2, g)
    de = torch.randn(B, T1, generator=g)
    dpi = _run_e_bwd(lib, imv.to(dev), e.to(dev), de.to(dev), tl.to(dev), ml.to(dev), B, T1, T2)
    torch.cuda.synchronize()
    fn = lambda t: R.aligned_positions(t, R.index_vector(tm, t.dtype), mm, tm, SIGMA_E)      # noqa: E731
    _check("efts_e_bwd", f"{B}x{T1}x{T2}", dpi, _grad(fn, imv, de, torch.float64), _grad(fn, imv, de, torch.float32))
    x = imv.to(dev)
    assert lib.efts_e_bwd(x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), SIGMA_E, x.data_ptr(), x.data_ptr(), 1, 4097, T2,
                          _st()) == -2
    assert b"LDS" in lib.efts_last_error()


def _imv_inputs(T2, seed):
    """5 items: [0] full length, [1] full length with a falling tail (the cumsum's maximum is a plateau), [2] never rises (clamp),
    [3] mel_len < T2 with a soft index that keeps rising beyond it, [4] text_len 1"""
    g = torch.Generator().manual_seed(seed)
    B = 5
    tl = torch.tensor([40, 23, 17, 31, 1], dtype=torch.int32)
    ml = torch.tensor([T2, T2, T2, max(1, (2 * T2) // 3), max(1, T2 - 2)], dtype=torch.int32)
    s = R.rising_soft_index(tl, ml, T2, g).double()
    j = torch.arange(T2, dtype=torch.float64)
    top = max(1, (3 * T2) // 4)                                                    # item 1 falls from here on: a plateau of T2 - top frames
    s[1, top:] = s[1, top - 1] - 0.05 * (j[top:] - top + 1)
    s[2] = 20.0 - 0.01 * j - 0.3 * torch.rand(T2, generator=g, dtype=torch.float64).cumsum(0)
    return B, tl, ml, s.float(), top


@pytest.mark.parametrize("T2", [1, 33, 63, 64, 65, 211, 800, 4100])
def test_imv_bwd_vs_fp64(lib, T2):
    """efts_imv_bwd: dsoft_idx = d <pi(s), dpi> / ds through imv_generator's relu-diff / cumsum / mask / max-normalise.
    One wave per item, ceil(T2 / 64) frames per lane: T2 < 64 leaves lanes empty, 64 gives every lane one frame, 65 gives lane 32 the
    last and 31 lanes none; item 0 and 1 end on the last frame so the last lanes of the suffix sum carry weight."""
    dev = _dev()
    B, tl, ml, s, top = _imv_inputs(T2, T2 + 17)
    mm = R.non_pad_mask(ml, T2)
    imv = R.imv_from_soft_index(s.double(), mm, tl).float()
    g = torch.Generator().manual_seed(T2)
    dpi = torch.randn(B, T2, generator=g) * mm                                      # efts_e_bwd leaves 0 at j >= mel_len
    if T2 >= 33:                                                                    # the inputs are what the docstring says they are
        u1 = torch.relu(s[1, 1:].double() - s[1, :-1].double()).cumsum(0)
        first = int((u1 == u1.max()).nonzero()[0]) + 1
        assert T2 - first >= 3 and bool((imv[1, first:] == imv[1, first]).all()) and float(imv[1, first - 1]) < float(imv[1, first])
        assert float(imv[2].abs().max()) == 0.0 and bool((s[3, int(ml[3]):].diff() > 0).any())
    ds = torch.full((B, T2), 7.0, device=dev)
    d = [t.to(dev) for t in (s, imv, dpi, tl, ml)]                                  # (kept alive until the kernel has run)
    O.imv_bwd(d[0], d[1], d[2], d[3], d[4], ds, B, T2)
    torch.cuda.synchronize()
    fn = lambda t: R.imv_from_soft_index(t, mm, tl)                                 # noqa: E731
    ref64, ref32 = _grad(fn, s, dpi, torch.float64), _grad(fn, s, dpi, torch.float32)
    _check("efts_imv_bwd", f"T2={T2}", ds, ref64, ref32)
    ds = ds.cpu()
    for b in range(4):                                                              # per item too: one item's error must not hide behind another's range
        if float(ref64[b].abs().max()) > 0:
            _check("efts_imv_bwd", f"T2={T2}[item {b}]", ds[b], ref64[b], ref32[b])
    assert bool((ds[2] == 0).all()) and bool((ref64[2] == 0).all())                  # never rises: clamp branch, exactly 0
    assert bool((ds[4] == 0).all()) and bool((ref64[4] == 0).all())                  # text_len 1: scale 0
    assert bool((ds[3, int(ml[3]):] == 0).all())                                     # beyond mel_len


def _unpack_plane(pl, B, Tp, T, kp):
    """rows (b * Tp + j), j < T, of a bf16x3 plane [B * Tp][ld bytes] -> hi + lo as float32 [B, T, kp]: every 128-byte chunk holds
    32 hi then 32 lo bf16 (tests/test_align_gpu.py, test_pack_vt_layout_both_kernels)"""
    nchunk = kp // 32
    w = pl.cpu().view(torch.bfloat16).view(B, Tp, -1)[:, :T, :nchunk * 64].reshape(B, T, nchunk, 2, 32).float()
    return (w[:, :, :, 0] + w[:, :, :, 1]).reshape(B, T, kp)


def _raw_plane(buf, ld):
    """a caller-owned byte buffer [rows, ld] as the bf16x3 output plane of a wrapper (what ops.Plane carries, with this test's own ld)"""
    return SimpleNamespace(ptr=buf.data_ptr(), ld=ld, split=2)


def _run_attn_bwd(lib, scores, ld, sidx, ds, tl, ml, B, T1, T2, ldd, pad_ldp):
    dev = _dev()
    kp = (T1 + 31) // 32 * 32
    T2p, ldp = T2 + 2, kp * 4 + pad_ldp
    dS = torch.full((B, T2, ldd), 7.0, device=dev)
    pl = torch.full((B * T2p, ldp), 0xAB, dtype=torch.uint8, device=dev)
    O.attn_bwd(scores, ld, sidx, ds, tl, ml, dS, ldd, _raw_plane(pl, ldp), B, T1, T2, T2p)
    return dS, pl, kp, T2p, ldp


def _check_attn_outputs(case, dS, pl, ref64, ref32, mm, B, T1, T2, kp, T2p, ldp, chain=False):
    dS = dS.cpu()
    _check("chain" if chain else "efts_attn_bwd", case, dS[:, :, :T1], ref64, ref32, chain)
    assert bool((dS[:, :, T1:] == 7.0).all())                                       # columns T1 <= i < ldd are not the kernel's
    assert bool((dS[:, :, :T1][~mm] == 0).all())                                    # dead frames: exactly 0
    both = _unpack_plane(pl, B, T2p, T2, kp)
    scale = float(dS[:, :, :T1].abs().max())
    assert float((both[:, :, :T1] - dS[:, :, :T1]).abs().max()) <= 2.0 ** -16 * scale
    assert bool((both[:, :, T1:] == 0).all()) and bool((both[~mm] == 0).all())       # pad columns and dead frames: exactly 0
    raw = pl.cpu().view(B, T2p, ldp)
    assert bool((raw[:, T2:] == 0xAB).all()) and bool((raw[:, :, kp * 4:] == 0xAB).all())   # gap rows and bytes past the chunks: untouched


@pytest.mark.parametrize("B,T1,T2,ldx", [(3, 37, 211, 3), (2, 128, 130, 0), (2, 63, 97, 1), (3, 5, 64, 4), (2, 31, 33, 0), (2, 203, 300, 5),
                                         (3, 1, 33, 2)])
def test_attn_bwd_vs_fp64(lib, B, T1, T2, ldx):
    """efts_attn_bwd: dscores = d <soft index(scores), ds> / dscores through scaled_dot_attention's masked softmax, in fp32 and as the
    bf16x3 operand plane.  T1 mod 32 = 5, 0, 31, 5, 31, 11, 1; row strides of scores / dscores / plane larger than needed (ldx)."""
    dev = _dev()
    g, tl, ml = _lengths(B, T1, T2, T1 * 1000 + T2 + 2)
    tm, mm = R.non_pad_mask(tl, T1), R.non_pad_mask(ml, T2)
    both = tm[:, :, None] & mm[:, None, :]
    ld, ldd = T1 + ldx, T1 + 2 * ldx
    scores = R.scores_for(tl, ml, T1, T2, g, ld=ld)
    s32 = scores[:, :, :T1].contiguous()
    fn = lambda t: R.soft_index(R.attention_from_scores(t, tm).masked_fill(~both, 0.0), R.index_vector(tm, t.dtype))   # noqa: E731
    sidx = fn(s32.double()).float()
    ds = torch.randn(B, T2, generator=g)
    dS, pl, kp, T2p, ldp = _run_attn_bwd(lib, scores.to(dev), ld, sidx.to(dev), ds.to(dev), tl.to(dev), ml.to(dev), B, T1, T2, ldd, 128 if ldx else 0)
    torch.cuda.synchronize()
    _check_attn_outputs(f"{B}x{T1}x{T2}", dS, pl, _grad(fn, s32, ds, torch.float64), _grad(fn, s32, ds, torch.float32), mm, B, T1, T2, kp, T2p, ldp)


@pytest.mark.parametrize("B,T1,T2", [(3, 37, 211), (2, 128, 800), (2, 203, 1500)])
def test_alignment_backward_chain_vs_fp64(lib, B, T1, T2):
    """efts_alpha_bwd -> efts_e_bwd -> efts_imv_bwd -> efts_attn_bwd back to back on the device against the float64 gradient of the whole
    block (scores -> alpha -> soft index -> pi -> e -> alpha') with respect to the scores; e32 is the whole chain in float32.

    The kernels take their stage inputs rounded from float64, so a relu(s_j - s_{j-1}) decision of theirs could differ from the reference's
    only where two neighbouring soft indices are closer than an ulp (1.5e-5 at 203): the inputs are asserted to keep 1e-4 between them.

    The condition 8 * e32 <= 2e-4 of the single-stage tests can not be asserted here.  Starting from the scores, float32 itself is at
    2e-5 ... 1.1e-4 at (2, 128, 800) and (2, 203, 1500) whatever the seed (eight seeds each; 3e-6 ... 8e-6 at (3, 37, 211)): the soft index
    has magnitude T1, so its float32 rounding (7.6e-6 at 128) enters the factor (i - s_j) = O(1) of the score gradient directly, on top
    of the 1e-5 ... 3.6e-5 of the three stages behind it.  What the condition is for -- a bound that can not grow until it hides an
    error -- is kept by capping the bound instead: the chain must be within min(max(8 * e32, 2e-6), 2e-4)."""
    dev = _dev()
    g = torch.Generator().manual_seed(T1 * 1000 + T2 + 3)
    tl, ml = R.ragged_lengths(B, T1, g), R.ragged_lengths(B, T2, g)
    scores = R.scores_for(tl, ml, T1, T2, g)
    blk = R.alignment_block(scores.double(), tl, ml, SIGMA, SIGMA_E)
    mm = blk["mel_mask"]
    assert float(blk["soft_idx"].diff(dim=1).abs()[mm[:, 1:]].min()) >= 1e-4
    dA = _upstream_dalpha(B, T1, T2, mm, g)
    f32 = {k: blk[k].float().to(dev) for k in ("soft_idx", "imv", "e", "ralpha")}
    tld, mld = tl.to(dev), ml.to(dev)
    _, de = _run_alpha_bwd(lib, f32["ralpha"], dA.to(dev), f32["e"], tld, mld, B, T1, T2)
    dpi = _run_e_bwd(lib, f32["imv"], f32["e"], de, tld, mld, B, T1, T2)
    dsx = torch.full((B, T2), 7.0, device=dev)
    O.imv_bwd(f32["soft_idx"], f32["imv"], dpi, tld, mld, dsx, B, T2)
    dS, pl, kp, T2p, ldp = _run_attn_bwd(lib, scores.to(dev), T1, f32["soft_idx"], dsx, tld, mld, B, T1, T2, T1, 0)
    torch.cuda.synchronize()
    fn = lambda t: R.alignment_block(t, tl, ml, SIGMA, SIGMA_E)["ralpha"]           # noqa: E731
    _check_attn_outputs(f"chain {B}x{T1}x{T2}", dS, pl, _grad(fn, scores, dA, torch.float64), _grad(fn, scores, dA, torch.float32), mm, B, T1, T2,
                        kp, T2p, ldp, chain=True)


# =====================================================================================================================
# embedding, loss
# =====================================================================================================================
@pytest.mark.parametrize("c", [128, 512])
def test_embed_bwd_vs_fp64(lib, c):
    """efts_embed_bwd: dtable.index_add_(ids, g) into a non-zero table; repeated ids inside one item and across items, an id that occurs
    once, the first and the last symbol, and gap rows (Tp > T) holding 1e30 that must never reach the table."""
    dev = _dev()
    B, T, Tp, nsym = 3, 23, 25, 76
    g = torch.Generator().manual_seed(c)
    ids = torch.randint(1, nsym - 1, (B, T), generator=g)
    ids[ids == 33] = 34
    ids[ids == 60] = 61
    ids[0, 0], ids[0, 1], ids[2, 5] = 0, nsym - 1, 33                               # 33: once; 60: never
    ids[0, 3:9], ids[1, 2], ids[1, 7], ids[2, 0] = 5, 5, 5, 5
    rows = torch.full((B, Tp, c), 1e30)
    rows[:, :T] = torch.randn(B, T, c, generator=g)
    table = torch.randn(nsym, c, generator=g)
    out = table.clone().to(dev)
    ids_d, rows_d = ids.to(dev), rows.to(dev)
    O.embed_bwd(ids_d, rows_d.data_ptr(), out, B, T, Tp, c)
    torch.cuda.synchronize()
    valid = rows[:, :T].reshape(B * T, c)
    ref64 = table.double().index_add_(0, ids.reshape(-1), valid.double())
    ref32 = table.clone().index_add_(0, ids.reshape(-1), valid)
    _check("efts_embed_bwd", f"c={c}", out, ref64, ref32)
    out = out.cpu()
    assert torch.equal(out[60], table[60])                                          # a symbol that does not occur: bit-identical
    assert torch.equal(out[33], (table[33].double() + rows[2, 5].double()).float())   # one occurrence: one rounding


def _loss_inputs(ldm, seed):
    B, T1, T1p, T2, T2p, odim = 3, 37, 39, 211, 213, 80
    g = torch.Generator().manual_seed(seed)
    tl, ml = R.ragged_lengths(B, T1, g, last=1), R.ragged_lengths(B, T2, g)
    mel = torch.full((B, T2p, ldm), 1e30)                                            # gap rows and columns >= odim are never read
    mel[:, :T2, :odim] = torch.randn(B, T2, odim, generator=g)
    speech = torch.randn(B, T2, odim, generator=g)
    dur = torch.full((B, T1p), 1e30)
    dur[:, :T1] = torch.randn(B, T1, generator=g)
    lde = torch.randn(B, T1, generator=g)
    lde[0, 3], lde[0, 20], lde[1, 0] = dur[0, 3], dur[0, 20], dur[1, 0]               # exact ties on live tokens
    return B, T1, T1p, T2, T2p, odim, tl, ml, mel, speech, dur, lde


@pytest.mark.parametrize("gscale", [None, 1.0, 0.5])
@pytest.mark.parametrize("ldm", [80, 96])
def test_loss_bwd_vs_fp64(lib, ldm, gscale):
    """efts_loss_bwd: d loss / d mel_pred (fp32 and bf16x3 plane) and d loss / d dur_pred of the masked L2 + L1 of the oracle's forward,
    times the device scalar gscale (NULL = 1); ragged lengths, row spaces with gap rows, ldm > odim; sign(0) = 0 on an exact tie."""
    dev = _dev()
    B, T1, T1p, T2, T2p, odim, tl, ml, mel, speech, dur, lde = _loss_inputs(ldm, 7)
    tm, mm = R.non_pad_mask(tl, T1), R.non_pad_mask(ml, T2)
    kp = 96
    ldp = kp * 4
    dmel = torch.full((B, T2p, odim), 7.0, device=dev)
    pl = torch.full((B * T2p, ldp), 0xAB, dtype=torch.uint8, device=dev)
    ddur = torch.full((B, T1p), 7.0, device=dev)
    gs = None if gscale is None else torch.tensor([gscale], device=dev)
    d = [t.to(dev) for t in (mel, speech, ml, dur, lde, tl)]
    O.loss_bwd(d[0].data_ptr(), ldm, d[1], d[2], d[3], d[4], d[5], gs, dmel.data_ptr(), _raw_plane(pl, ldp), ddur, B, T1, T1p, T2, T2p, odim)
    torch.cuda.synchronize()

    def grads(dtype):
        m = mel[:, :T2, :odim].to(dtype).requires_grad_(True)
        d = dur[:, :T1].to(dtype).requires_grad_(True)
        loss = sum(R.masked_losses(m, speech.to(dtype), d, lde.to(dtype), mm, tm)) * (1.0 if gscale is None else gscale)
        return torch.autograd.grad(loss, (m, d))
    (gm64, gd64), (gm32, gd32) = grads(torch.float64), grads(torch.float32)
    case = f"ldm={ldm} gscale={gscale}"
    dmel, ddur = dmel.cpu(), ddur.cpu()
    _check("efts_loss_bwd.dmel", case, dmel[:, :T2], gm64, gm32)
    _check("efts_loss_bwd.ddur", case, ddur[:, :T1], gd64, gd32)
    assert bool((dmel[:, T2:] == 0).all()) and bool((dmel[:, :T2][~mm] == 0).all())   # gap rows and padded frames: exactly 0
    assert bool((ddur[:, T1:] == 0).all()) and bool((ddur[:, :T1][~tm] == 0).all())
    assert float(ddur[0, 3]) == 0.0 and float(ddur[0, 20]) == 0.0 and float(ddur[1, 0]) == 0.0     # ties
    live = tm.clone()
    live[0, 3] = live[0, 20] = live[1, 0] = False
    assert bool((ddur[:, :T1][live] != 0).all())
    assert bool((torch.sign(ddur[:, :T1]) == torch.sign(gd64)).all())
    both = _unpack_plane(pl, B, T2p, T2p, kp)
    assert float((both[:, :, :odim] - dmel).abs().max()) <= 2.0 ** -16 * float(dmel.abs().max())
    assert bool((both[:, :, odim:] == 0).all())


@pytest.mark.parametrize("ldm", [80, 96, 81])
def test_masked_losses_vs_fp64(lib, ldm):
    """efts_masked_losses: (loss, mel L2, duration L1) of the oracle's forward; ldm = 81 takes the scalar path of the first stage"""
    dev = _dev()
    B, T1, T1p, T2, T2p, odim, tl, ml, mel, speech, dur, lde = _loss_inputs(ldm, 11)
    tm, mm = R.non_pad_mask(tl, T1), R.non_pad_mask(ml, T2)
    out3 = torch.full((3,), 7.0, device=dev)
    ws = torch.zeros(lib.efts_losses_workspace_bytes() // 4, device=dev)
    d = [t.to(dev) for t in (mel, speech, ml, dur, lde, tl)]
    _call("efts_masked_losses", lib.efts_masked_losses(d[0].data_ptr(), ldm, d[1].data_ptr(), d[2].data_ptr(),
                                                       d[3].data_ptr(), d[4].data_ptr(), d[5].data_ptr(), out3.data_ptr(),
                                                       ws.data_ptr(), B, T1, T1p, T2, T2p, odim, _st()))
    torch.cuda.synchronize()

    def values(dtype):
        a, b = R.masked_losses(mel[:, :T2, :odim].to(dtype), speech.to(dtype), dur[:, :T1].to(dtype), lde.to(dtype), mm, tm)
        return torch.stack([a + b, a, b])
    v64, v32 = values(torch.float64), values(torch.float32)
    out3 = out3.cpu()
    for k, name in enumerate(("loss", "mel", "dur")):
        _check(f"efts_masked_losses.{name}", f"ldm={ldm}", out3[k:k + 1], v64[k:k + 1], v32[k:k + 1])


# =====================================================================================================================
# LayerNorm of the duration predictor (drop_p = 0)
# =====================================================================================================================
LN_EPS = 1e-12
LN_CASES = [(rows, c) for c in (256, 512, 2048) for rows in (1, 7, 8, 9)] + [(4100, 512), (4100, 2048)]


def _ln_inputs(rows, c, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(rows, c, generator=g)
    gamma = 1.0 + 0.1 * torch.randn(c, generator=g)
    beta = 0.1 * torch.randn(c, generator=g)
    rm = (torch.rand(rows, generator=g) > 0.3).float()                               # dead rows
    if rows > 1:
        rm[0], rm[rows - 1] = 1.0, 0.0
    return g, z, gamma, beta, rm


@pytest.mark.parametrize("rows,c", LN_CASES)
def test_layernorm_rows_and_dot_vs_fp64(lib, rows, c):
    """efts_layernorm_rows: LN_c(x) gamma + beta, times rowmask; efts_layernorm_dot: (LN_c(x) . w + b) rowmask; x = relu(z) as in the model"""
    dev = _dev()
    g, z, gamma, beta, rm = _ln_inputs(rows, c, rows * 7 + c)
    w, b = torch.randn(c, generator=g) / c ** 0.5, torch.randn(1, generator=g)
    x = torch.relu(z)
    xd, gd, bd, rmd, wd, bbd = x.to(dev), gamma.to(dev), beta.to(dev), rm.to(dev), w.to(dev), b.to(dev)
    y = torch.full((rows, c), 7.0, device=dev)
    _call("efts_layernorm_rows", lib.efts_layernorm_rows(xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), LN_EPS, rmd.data_ptr(), y.data_ptr(), None, 0,
                                                         rows, c, 2, 0.0, 0, None, _st()))
    out = torch.full((rows,), 7.0, device=dev)
    _call("efts_layernorm_dot", lib.efts_layernorm_dot(xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), LN_EPS, wd.data_ptr(), bbd.data_ptr(),
                                                       rmd.data_ptr(), 0, 1.0, out.data_ptr(), rows, c, 0.0, 0, None, _st()))
    torch.cuda.synchronize()

    def ref(dtype):
        ln = R.relu_layernorm(z.to(dtype), gamma.to(dtype), beta.to(dtype), LN_EPS)
        return ln * rm.to(dtype)[:, None], (ln @ w.to(dtype) + b.to(dtype)) * rm.to(dtype)
    (y64, o64), (y32, o32) = ref(torch.float64), ref(torch.float32)
    _check("efts_layernorm_rows", f"{rows}x{c}", y, y64, y32)
    _check("efts_layernorm_dot", f"{rows}x{c}", out, o64, o32)
    assert bool((y.cpu()[rm == 0] == 0).all()) and bool((out.cpu()[rm == 0] == 0).all())


@pytest.mark.parametrize("form", ["dy", "ddur", "ddur_rowmask"])
@pytest.mark.parametrize("rows,c", LN_CASES)
def test_layernorm_bwd_vs_fp64(lib, rows, c, form):
    """efts_layernorm_bwd through relu -> LayerNorm (-> Linear(c, 1)): dz, and dgamma, dbeta, the conv-bias gradient (column sums of dz), dw, db
    ACCUMULATED into non-zero buffers.  8 rows per block, 4 waves: rows 1, 7, 8, 9 end inside / at / just past the first block.
    `dy` form: upstream [rows, c] with a rowmask that has dead rows; `ddur` form: upstream [rows] times w, 0 on dead rows as efts_loss_bwd leaves it."""
    dev = _dev()
    g, z, gamma, beta, rm = _ln_inputs(rows, c, rows * 11 + c + len(form))
    w, b = torch.randn(c, generator=g) / c ** 0.5, torch.randn(1, generator=g)
    dy = torch.randn(rows, c, generator=g)
    # (standard normal around 0.5, not 0: db = sum ddur is ONE number, and the metric is relative to it.  Around 0 it is ~sqrt(rows) while the
    #  kernel's 4 atomic adds per block walk through partial sums of that same size in arbitrary order -- 2052 roundings of half an ulp of 64 against a
    #  result of 7 measured 5e-6 at 4100 x 2048, where torch's pairwise float32 sum is at 1e-7.  That is the conditioning of the sum, not the kernel.)
    ddur = (0.5 + torch.randn(rows, generator=g)) * rm
    init = {k: torch.randn(c if k != "db" else 1, generator=g) for k in ("dgamma", "dbeta", "dbias", "dw", "db")}
    acc = {k: v.clone().to(dev) for k, v in init.items()}
    x = torch.relu(z).to(dev)
    dz = torch.full((rows, c), 7.0, device=dev)
    gd, bd, wd, rmd, dyd, ddurd = gamma.to(dev), beta.to(dev), w.to(dev), rm.to(dev), dy.to(dev), ddur.to(dev)
    if form == "dy":
        O.layernorm_bwd(x.data_ptr(), gd, bd, LN_EPS, dyd.data_ptr(), None, None, rmd.data_ptr(), dz.data_ptr(), None,
                        acc["dgamma"], acc["dbeta"], acc["dbias"], None, None, rows, c)
    else:
        O.layernorm_bwd(x.data_ptr(), gd, bd, LN_EPS, None, ddurd, wd, rmd.data_ptr() if form == "ddur_rowmask" else None, dz.data_ptr(), None,
                        acc["dgamma"], acc["dbeta"], acc["dbias"], acc["dw"], acc["db"], rows, c)
    torch.cuda.synchronize()

    def ref(dtype):
        t = lambda v: v.to(dtype)                                                    # noqa: E731
        zz, bias = t(z).requires_grad_(True), torch.zeros(c, dtype=dtype, requires_grad=True)
        gm, bt, ww, bb = (t(v).requires_grad_(True) for v in (gamma, beta, w, b))
        ln = R.relu_layernorm(zz + bias, gm, bt, LN_EPS)
        if form == "dy":
            loss = (ln * t(rm)[:, None] * t(dy)).sum()
            gz, ggm, gbt, gbias = torch.autograd.grad(loss, (zz, gm, bt, bias))
            gw = gb = None
        else:
            loss = ((ln @ ww + bb) * t(ddur)).sum()
            gz, ggm, gbt, gbias, gw, gb = torch.autograd.grad(loss, (zz, gm, bt, bias, ww, bb))
        out = dict(dz=gz, dgamma=t(init["dgamma"]) + ggm, dbeta=t(init["dbeta"]) + gbt, dbias=t(init["dbias"]) + gbias)
        if gw is not None:
            out.update(dw=t(init["dw"]) + gw, db=t(init["db"]) + gb)
        return out
    r64, r32 = ref(torch.float64), ref(torch.float32)
    case = f"{form} {rows}x{c}"
    _check("efts_layernorm_bwd.dz", case, dz, r64["dz"], r32["dz"])
    for k in ("dgamma", "dbeta", "dbias", "dw", "db"):
        if k in r64:
            _check(f"efts_layernorm_bwd.{k}", case, acc[k], r64[k], r32[k])
    assert bool((dz.cpu()[rm == 0] == 0).all())
    if form == "dy":                                                                 # not this form's outputs: untouched
        assert torch.equal(acc["dw"].cpu(), init["dw"]) and torch.equal(acc["db"].cpu(), init["db"])


# =====================================================================================================================
# reductions and the gradient scale
# =====================================================================================================================
@pytest.mark.parametrize("T", [1, 63, 64, 255, 256, 257, 1000])
def test_cumsum_rows_vs_fp64(lib, T):
    """efts_cumsum_rows: 256 threads with ceil(T / 256) elements each; durations are positive"""
    dev = _dev()
    B = 3
    x = torch.rand(B, T, generator=torch.Generator().manual_seed(T)) * 12.0 + 0.5
    y = torch.full((B, T), -1.0, device=dev)
    xd = x.to(dev)
    _call("efts_cumsum_rows", lib.efts_cumsum_rows(xd.data_ptr(), y.data_ptr(), B, T, _st()))
    torch.cuda.synchronize()
    _check("efts_cumsum_rows", f"T={T}", y, x.double().cumsum(1), x.cumsum(1))


BIG_N = [1, 3, 4, 1023, 1024 * 1024 + 1, 20_000_003]


@pytest.mark.parametrize("n", BIG_N)
def test_sumsq_vs_fp64(lib, n):
    """efts_sumsq: out1 += sum g^2 (float4 body + scalar tail; n mod 4 = 1, 3, 0, 3, 1, 3), deterministic: two calls, identical bits"""
    dev = _dev()
    gcpu = torch.randn(n, generator=torch.Generator().manual_seed(n % 1000))
    gdev = gcpu.to(dev)
    ws = torch.zeros(lib.efts_sumsq_workspace_bytes() // 4, device=dev)
    outs = []
    for _ in range(2):
        out = torch.tensor([3.25], device=dev)
        _call("efts_sumsq", lib.efts_sumsq(gdev.data_ptr(), n, out.data_ptr(), ws.data_ptr(), _st()))
        torch.cuda.synchronize()
        outs.append(out.cpu())
    assert torch.equal(outs[0], outs[1])
    ref64 = (3.25 + (gcpu.double() ** 2).sum()).reshape(1)
    ref32 = (torch.tensor(3.25) + (gcpu ** 2).sum()).reshape(1)
    _check("efts_sumsq", f"n={n}", outs[0], ref64, ref32)


@pytest.mark.parametrize("n", BIG_N)
def test_scale_unless_one(lib, n):
    """efts_scale_unless_one: x *= *scale; 1 leaves every bit alone (the pass is skipped), 0.5 and 3 give the correctly rounded product"""
    dev = _dev()
    xcpu = torch.randn(n + 5, generator=torch.Generator().manual_seed(n % 999))
    for s in (1.0, 0.5, 3.0):
        buf = xcpu.clone().to(dev)                                                   # 5 elements past n: not the kernel's
        sc = torch.tensor([s], device=dev)
        O.scale_unless_one(buf, n, sc)
        torch.cuda.synchronize()
        got = buf.cpu()
        assert torch.equal(got[n:], xcpu[n:])
        if s == 1.0:
            assert torch.equal(got.view(torch.int32), xcpu.view(torch.int32))
        else:
            assert torch.equal(got[:n], (xcpu[:n].double() * s).float())
