"""GPU: precision="fp32" -- operand format 3 (exact fp32 planes) contracted on v_mfma_f32_32x32x2_f32 by efts_gemm's generic kernel.

The plane producers write the value they computed, unrounded; the contraction is an fp32 fmaf chain, so the error bound is the one of
an fp32 dot product (|got - ref| <= 1e-6 * sum_k |a_k b_k|), and the model is held to the bounds a second fp32 CPU formulation meets
(tests/test_oracle_golden.py TOL) -- not to the 1e-3 of the bf16x3 mode."""
import os

import numpy as np
import pytest
import torch

from oracle import efts_oracle as O
from oracle import hifigan_oracle as HO

pytestmark = pytest.mark.gpu

# fp32 re-association noise between two CPU formulations of the same maths (tests/test_oracle_golden.py)
TOL = dict(loss=2e-5, mel_loss=2e-5, dur_loss=2e-5, imv=3e-4, e=1e-3, dur_pred=2e-5,
           log_delta_e=3e-4, mel_pred=5e-4, reconst_alpha=1e-4)
HIFIGAN_V1 = dict(resblock="1", upsample_rates=[8, 8, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4], upsample_initial_channel=512,
                  resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 5]], num_mels=80)
SPLIT = 3


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _golden(golden_dir, name):
    return np.load(os.path.join(golden_dir, name + ".npz"))


@pytest.fixture(scope="module")
def model():
    from efficient_tts_amd import EfficientTTSCNN
    from efficient_tts_amd import lib as L
    L.load()
    L.require_device()
    m = EfficientTTSCNN(num_symbols=76, dropout_rate=0.0, use_masking=True, use_weighted_masking=False, sigma=0.01, precision="fp32")
    m.load_state_dict(O.fill_params())
    return m.to(_dev()).eval()


# ------------------------------------------------------------------ 1. the plane producer
@pytest.mark.parametrize("B,T,c", [(2, 37, 80), (1, 130, 512), (3, 5, 200)])
def test_pack_rows_format3_is_the_input(B, T, c):
    from efficient_tts_amd import lib as L, ops as P
    dev = _dev()
    x = torch.randn(B, T, c, generator=torch.Generator().manual_seed(B * 100 + T + c)).to(dev)
    rs = P.Rows(B, T)
    pl = P.Plane.for_rows(rs, c, SPLIT, dev)
    pl.buf.fill_(0xAB)                                  # every byte of the rows must be written (gap rows, padding k) -- guards left alone
    pl.buf[:L.GUARD_LO].zero_()
    P.pack_rows(x, None, pl, rs)
    torch.cuda.synchronize()
    rows = pl.buf[L.GUARD_LO:L.GUARD_LO + rs.rows].view(torch.float32).view(B, rs.Tp, pl.nchunk * 32)
    assert torch.equal(rows[:, :T, :c], x)
    assert float(rows[:, :T, c:].abs().max() if pl.nchunk * 32 > c else 0.0) == 0.0       # padding k
    assert float(rows[:, T:].abs().max()) == 0.0                                          # gap rows


# ------------------------------------------------------------------ 2. the contraction
def _conv_case(taps, cin, cout, B, T, dil=1, act="leaky", resid=True, mask=True, seed=0):
    """efts_gemm format 3 vs fp64 on a (dilated) convolution over a padded row space; returns what the checks need"""
    from efficient_tts_amd import lib as L, ops as P
    dev = _dev()
    g = torch.Generator().manual_seed(seed + taps * 1000 + cin + T + dil)
    x = torch.randn(B, T, cin, generator=g)
    w = torch.randn(cout, cin, taps, generator=g) * 0.05
    bias = torch.randn(cout, generator=g)
    res = torch.randn(B, T, cout, generator=g)
    pad = (taps - 1) // 2 * dil
    rs = P.Rows(B, T, gap=max(L.GAP, pad))
    guard = max(L.GUARD_LO, pad)                        # zero rows in front of row 0 for the widest tap reach
    a = P.Plane(rs.alloc + guard, cin, SPLIT, dev, guard_lo=guard)
    P.pack_rows(x.to(dev), None, a, rs)
    pw = P.PackedWeight(cout, cin, taps, SPLIT, dev)
    pw.pack(w.to(dev).contiguous())
    resid_rows = P.F32Rows(rs, cout, dev)
    resid_rows.view().copy_(res.to(dev))
    keep = torch.ones(B, T)
    if mask:
        keep = (torch.rand(B, T, generator=g) > 0.2).float()
    rowmask = torch.zeros(B, rs.Tp)
    rowmask[:, :T] = keep
    rowmask = rowmask.reshape(-1).to(dev)
    out = P.F32Rows(rs, cout, dev)
    outp = P.Plane.for_rows(rs, cout, SPLIT, dev)
    actid = {"leaky": L.ACT_LEAKY, "tanh": L.ACT_TANH, "none": L.ACT_NONE}[act]
    P.gemm(a=a, b_ptr=pw.ptr, ldb=pw.ld, b_tap_stride=pw.tap_stride, taps=taps, m=rs.rows, n=cout, act=actid, slope=0.1,
           bias=bias.to(dev), resid_ptr=resid_rows.ptr if resid else None, ldr=cout, rowmask_ptr=rowmask.data_ptr(),
           out_f32_ptr=out.ptr, ldo=cout, out_plane=outp, dilation=dil, plane_act=True, plane_slope=0.2)
    torch.cuda.synchronize()
    xd, wd = x.double().transpose(1, 2), w.double()
    z = torch.nn.functional.conv1d(xd, wd, bias.double(), padding=pad, dilation=dil).transpose(1, 2)
    mag = torch.nn.functional.conv1d(xd.abs(), wd.abs(), bias.double().abs(), padding=pad, dilation=dil).transpose(1, 2)
    if act == "leaky":
        z = torch.nn.functional.leaky_relu(z, 0.1)
    elif act == "tanh":
        z = torch.tanh(z)
    if resid:
        z = z + res.double()
        mag = mag + res.double().abs()
    ref = z * keep[..., None].double()
    got = out.view().cpu()
    plane = outp.buf[L.GUARD_LO:L.GUARD_LO + rs.rows].view(torch.float32).view(B, rs.Tp, outp.nchunk * 32)[:, :T, :cout].cpu()
    return got, ref, mag, keep, plane


@pytest.mark.parametrize("taps,cin,cout,B,T,dil", [(5, 512, 512, 3, 70, 1), (3, 512, 512, 2, 131, 1), (1, 80, 512, 2, 50, 1),
                                                   (1, 512, 80, 1, 300, 1), (5, 512, 512, 1, 1, 1),
                                                   (7, 256, 128, 1, 200, 3), (9, 128, 256, 2, 90, 3), (11, 64, 64, 1, 400, 5),
                                                   (11, 200, 96, 1, 150, 3), (3, 72, 160, 2, 33, 5)])
def test_gemm_format3_vs_fp64(taps, cin, cout, B, T, dil):
    got, ref, mag, keep, plane = _conv_case(taps, cin, cout, B, T, dil)
    err = (got.double() - ref).abs()
    bound = 1e-6 * mag
    print(f"taps {taps} dil {dil} K {cin * taps}: max err {float(err.max()):.3e}, max err / sum|ab| {float((err / mag.clamp_min(1e-30)).max()):.3e}")
    assert bool((err <= bound).all())
    assert float(got[keep == 0].abs().max() if bool((keep == 0).any()) else 0.0) == 0.0      # masked rows exactly zero
    assert torch.equal(plane, torch.nn.functional.leaky_relu(got, 0.2))                      # plane_act: LeakyReLU of the fp32 output, bit for bit


@pytest.mark.parametrize("act", ["tanh", "none"])
def test_gemm_format3_activations_without_residual(act):
    got, ref, mag, keep, plane = _conv_case(3, 96, 64, 2, 77, 1, act=act, resid=False)
    err = (got.double() - ref).abs()
    assert bool((err <= 1e-6 * mag + (5e-7 if act == "tanh" else 0.0)).all()), float(err.max())
    assert torch.equal(plane, torch.nn.functional.leaky_relu(got, 0.2))


def test_gemm_format3_batched_product():
    """the alignment block's form: batch > 1 with per-item operand strides, K = T1 in partial chunks, alpha, row masks"""
    from efficient_tts_amd import ops as P
    dev = _dev()
    g = torch.Generator().manual_seed(11)
    B, M, N, K = 3, 150, 96, 45
    a = torch.randn(B, M, K, generator=g)
    b = torch.randn(B, N, K, generator=g)
    ap = P.Plane(B * M + 8 + 272, K, SPLIT, dev, guard_lo=8)
    bp = P.Plane(B * N + 8 + 272, K, SPLIT, dev, guard_lo=8)
    P.pack_rows(a.reshape(1, B * M, K).to(dev), None, ap, P.Rows(1, B * M, gap=0))
    P.pack_rows(b.reshape(1, B * N, K).to(dev), None, bp, P.Rows(1, B * N, gap=0))
    rm = (torch.rand(B, M, generator=g) > 0.3).float()
    out = torch.zeros(B, M, N, device=dev)
    P.gemm(a=ap, b_ptr=bp.ptr, ldb=bp.ld, m=M, n=N, batch=B, a_batch_stride=M * ap.ld, b_batch_stride=N * bp.ld, alpha=0.125,
           rowmask_ptr=rm.to(dev).data_ptr(), rowmask_batch_stride=M, out_f32_ptr=out.data_ptr(), ldo=N, out_batch_stride=M * N)
    torch.cuda.synchronize()
    ref = 0.125 * torch.bmm(a.double(), b.double().transpose(1, 2)) * rm[..., None].double()
    mag = 0.125 * torch.bmm(a.double().abs(), b.double().abs().transpose(1, 2))
    assert bool(((out.cpu().double() - ref).abs() <= 1e-6 * mag).all())
    assert float(out.cpu()[rm == 0].abs().max()) == 0.0


# ------------------------------------------------------------------ 3. the teacher-forced forward against the reference goldens
@pytest.mark.parametrize("case", ["fwd_tiny", "fwd_small", "fwd_full", "fwd_long"])
def test_forward_matches_reference_golden(golden_dir, model, case):
    g = _golden(golden_dir, case)
    dev = _dev()
    args = [torch.from_numpy(g[k]).to(dev) for k in ("text", "text_lengths", "speech", "speech_lengths")]
    with torch.no_grad():
        loss, stats, imv, ralpha, mel_pred, _ = model(*args)
        (_, _, _, _, _, _), extra = model._forward_impl(*args, keep=True)
    st, sa = int(g["mel_pred_stride"]), int(g["alpha_stride"])
    got = dict(loss=loss, mel_loss=stats["mel_loss"], dur_loss=stats["duration_loss"], imv=imv, mel_pred=mel_pred[:, ::st],
               reconst_alpha=ralpha[:, ::sa, ::sa], e=extra["e"], dur_pred=extra["dur_pred"], log_delta_e=extra["log_delta_e"])
    errs = {}
    for k, tol in TOL.items():
        ref = torch.from_numpy(np.asarray(g[k]))
        scale = max(1.0, float(ref.abs().max())) if k in ("loss", "mel_loss", "dur_loss") else 1.0
        errs[k] = float((torch.as_tensor(got[k]).detach().cpu().reshape(ref.shape) - ref).abs().max())
        assert errs[k] <= tol * scale, f"{case}:{k} max-abs {errs[k]:.3e} > {tol * scale:.1e}"
    print(case, {k: f"{v:.2e}" for k, v in errs.items()})
    # and against the oracle on the full tensors
    P = O.fill_params()
    ref = O.forward(P, *[torch.from_numpy(g[k]) for k in ("text", "text_lengths", "speech", "speech_lengths")])
    assert float((mel_pred.cpu() - ref["mel_pred"]).abs().max()) <= TOL["mel_pred"]
    assert float((ralpha.cpu() - ref["reconst_alpha"]).abs().max()) <= TOL["reconst_alpha"]
    assert float((imv.cpu() - ref["imv"]).abs().max()) <= TOL["imv"]


# ------------------------------------------------------------------ 4. free-running inference
def test_inference_matches_reference_golden(golden_dir, model):
    g = _golden(golden_dir, "inference_lj")
    dev = _dev()
    n_utt = len([k for k in g.files if k.startswith("t2_")])
    for n in range(n_utt):
        mel, ralpha = model.inference(torch.from_numpy(g[f"text{n}"]).to(dev))
        assert mel.shape[1] == int(g[f"t2_{n}"]), n
        assert float((mel.cpu()[:, ::2] - torch.from_numpy(g[f"mel_pred{n}"])).abs().max()) <= 1e-4, n
        assert float((ralpha.cpu()[:, ::4, ::4] - torch.from_numpy(g[f"reconst_alpha{n}"])).abs().max()) <= 1e-5, n


def test_batched_ragged_inference_equals_single_item(golden_dir, model):
    g = _golden(golden_dir, "inference_lj")
    dev = _dev()
    n_utt = len([k for k in g.files if k.startswith("t2_")])
    seqs = [torch.from_numpy(g[f"text{n}"])[0] for n in range(n_utt)]
    T1 = max(len(s) for s in seqs)
    text = torch.zeros(len(seqs), T1, dtype=torch.int64)
    for n, s in enumerate(seqs):
        text[n, :len(s)] = s
    lens = torch.tensor([len(s) for s in seqs])
    mel, mel_len, ralpha = model.inference_batch(text.to(dev), lens.to(dev))
    for n, s in enumerate(seqs):
        t2 = int(g[f"t2_{n}"])
        assert int(mel_len[n]) == t2
        one, ra1 = model.inference(s[None].to(dev))
        assert float((mel[n, :t2] - one[0]).abs().max()) <= 2e-4
        assert float(mel[n, t2:].abs().max()) == 0.0 if mel.shape[1] > t2 else True
        assert float((ralpha[n, :len(s), :t2] - ra1[0]).abs().max()) <= 1e-5


# ------------------------------------------------------------------ 5. config 5, the shape bf16x3 misses with the plain fill
def _oracle_fp64(P, text, tl, mel, sl):
    """the oracle's maths evaluated in float64 (its own float32 aranges promoted too): the exact result the two fp32 formulations are
    both approximations of"""
    arange, dtype = torch.arange, torch.get_default_dtype()

    def arange64(*a, **k):
        if k.get("dtype") == torch.float32:
            k["dtype"] = torch.float64
        return arange(*a, **k)
    torch.arange = arange64
    torch.set_default_dtype(torch.float64)
    try:
        return O.forward({k: v.double() for k, v in P.items()}, text, tl, mel.double(), sl)["mel_pred"]
    finally:
        torch.arange = arange
        torch.set_default_dtype(dtype)


def test_long_sequence_plain_fill_meets_the_absolute_bound():
    """config 5 at (200, 1500), B = 16, plain fill, |mel| ~ 15: the first two items within the absolute 1e-3, no rescaling of the mel
    head.  The checker is the oracle evaluated in float64: the fp32 oracle is itself 7.9e-4 off that result on item 0 (measured), so
    against the fp32 oracle the two fp32 formulations differ by their two roundings (1.01e-3 measured, printed below)."""
    from efficient_tts_amd import EfficientTTSCNN
    dev = _dev()
    T1, T2, B = 200, 1500, 16
    gen = torch.Generator().manual_seed(T1 * 10000 + T2)          # (the inputs of tests/test_gpu_fullsize.py's plain-fill case)
    text = torch.randint(0, 76, (B, T1), generator=gen)
    mel = torch.randn(B, T2, 80, generator=gen)
    tl = torch.randint(T1 // 2, T1 + 1, (B,), generator=gen); tl[0] = T1
    sl = torch.randint(T2 // 2, T2 + 1, (B,), generator=gen); sl[0] = T2
    P = O.fill_params()
    m = EfficientTTSCNN(num_symbols=76, dropout_rate=0.0, use_masking=True, use_weighted_masking=False, sigma=0.01, precision="fp32")
    m.load_state_dict(P)
    m = m.to(dev).eval()
    with torch.no_grad():
        mp = m(*[t.to(dev) for t in (text, tl, mel, sl)])[4].cpu()
        ref32 = O.forward(P, text[:2], tl[:2], mel[:2], sl[:2])["mel_pred"]
        ref64 = _oracle_fp64(P, text[:2], tl[:2], mel[:2], sl[:2])
    err64 = max(float((mp[b, :int(sl[b])].double() - ref64[b, :int(sl[b])]).abs().max()) for b in range(2))
    err32 = max(float((mp[b, :int(sl[b])] - ref32[b, :int(sl[b])]).abs().max()) for b in range(2))
    o32 = max(float((ref32[b, :int(sl[b])].double() - ref64[b, :int(sl[b])]).abs().max()) for b in range(2))
    print(f"(200, 1500) plain fill, fp32: mel max-abs {err64:.3e} vs the fp64 oracle, {err32:.3e} vs the fp32 oracle "
          f"(fp32 oracle vs fp64: {o32:.3e}), max |mel| {float(ref64.abs().max()):.2f}")
    assert float(ref64.abs().max()) > 5.0                 # (the point of the case: outputs beyond the LJSpeech range)
    assert err64 <= 1e-3


# ------------------------------------------------------------------ 6. the vocoder
def test_vocoder_fp32_matches_reference_golden(golden_dir):
    from efficient_tts_amd.vocoder import HiFiGANGenerator
    g = _golden(golden_dir, "hifigan_small")
    m = HiFiGANGenerator(HIFIGAN_V1, precision="fp32")
    m.load_state_dict(HO.fill_params())
    m = m.to(_dev()).eval()
    for name in ("a", "b"):
        y = m(torch.from_numpy(g[f"mel_{name}"]).to(_dev()))
        err = float(np.abs(y.cpu().numpy() - g[f"audio_{name}"]).max())
        print("fp32 vocoder", name, "max abs err", err)
        assert err <= 2e-5, (name, err)
    lens = [37, 12, 50, 1]
    mel = torch.randn(len(lens), 80, max(lens), generator=torch.Generator().manual_seed(7))
    y = m(mel.to(_dev()), torch.tensor(lens))
    for b, n in enumerate(lens):
        alone = m(mel[b:b + 1, :, :n].contiguous().to(_dev()))
        assert torch.equal(y[b, :, :n * 256], alone[0]), b
