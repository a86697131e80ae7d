"""CPU: the float64 references of tests/test_bwd_kernels_gpu.py are the oracle, and the backward entry points refuse bad shapes.

1. Every twin in tests/bwd_reference.py, evaluated in float32, equals the oracle function it transcribes (`torch.equal`: the
   operations are the same ones), on ragged random inputs; the two cut functions compose to the oracle's.
2. The twin's float64 autograd gradient passes `torch.autograd.gradcheck` on a small case away from the ReLU / abs / max kinks.
3. efts_alpha_bwd / efts_e_bwd / efts_imv_bwd / efts_attn_bwd / efts_embed_bwd return EFTS_ESHAPE with a message before any device
   work (the calls below run on a machine without a GPU; the pointers are never dereferenced).
"""
import os

import numpy as np
import pytest
import torch

import bwd_reference as R
from oracle import efts_oracle as O


def _case(B, T1, T2, seed):
    g = torch.Generator().manual_seed(seed)
    tl, ml = R.ragged_lengths(B, T1, g), R.ragged_lengths(B, T2, g)
    return g, tl, ml, R.non_pad_mask(tl, T1), R.non_pad_mask(ml, T2)


SHAPES = [(3, 37, 211), (2, 16, 64), (4, 9, 33), (2, 1, 5)]


@pytest.mark.parametrize("B,T1,T2", SHAPES)
def test_twins_equal_the_oracle_in_float32(B, T1, T2):
    g, tl, ml, tm, mm = _case(B, T1, T2, T1 * 31 + T2)
    C_ = 24
    q, k = torch.randn(B, T2, C_, generator=g), torch.randn(B, T1, C_, generator=g) * tm[:, :, None]
    a_o, a_t = O.scaled_dot_attention(q, k, tm), R.scaled_dot_attention(q, k, tm)
    assert torch.equal(a_o, a_t)
    p_o, p_t = O.index_vector(tm), R.index_vector(tm, torch.float32)
    assert p_o.dtype == p_t.dtype and torch.equal(p_o, p_t)
    both = tm[:, :, None] & mm[:, None, :]
    alpha = a_o.masked_fill(~both, 0.0)
    imv_o, imv_t = O.imv_generator(alpha, p_o, mm, tl), R.imv_generator(alpha, p_t, mm, tl)
    assert torch.equal(imv_o, imv_t)
    # the cut: a soft index that did not come from an attention, as the kernel tests feed it
    sidx = R.rising_soft_index(tl, ml, T2, g)
    assert torch.equal(R.imv_from_soft_index(R.soft_index(alpha, p_t), mm, tl), imv_o)
    assert R.imv_from_soft_index(sidx, mm, tl).dtype == torch.float32
    e_o, e_t = O.aligned_positions(imv_o, p_o, mm, tm, 0.5), R.aligned_positions(imv_t, p_t, mm, tm, 0.5)
    assert torch.equal(e_o, e_t)
    r_o, r_t = O.reconstruct_alignment(e_o, 0.01, mm, tm), R.reconstruct_alignment(e_t, 0.01, mm, tm)
    assert torch.equal(r_o, r_t)
    assert torch.equal(R.masked_ralpha(e_t, 0.01, mm, tm), r_o.masked_fill(~both, 0.0))
    # the whole block from the scores on
    s = torch.bmm(q, k.transpose(1, 2)) / float(C_) ** 0.5
    blk = R.alignment_block(s, tl, ml, 0.01, 0.5)
    assert torch.equal(blk["alpha"], alpha) and torch.equal(blk["imv"], imv_o) and torch.equal(blk["e"], e_o)
    assert torch.equal(blk["ralpha"], r_o.masked_fill(~both, 0.0))
    # float64 in, float64 out: nothing inside falls back to float32
    blk64 = R.alignment_block(s.double(), tl, ml, 0.01, 0.5)
    assert all(blk64[k].dtype == torch.float64 for k in ("alpha", "soft_idx", "imv", "e", "ralpha"))
    assert float((blk64["e"] - e_o.double()).abs().max()) <= 1e-3 * T2


def test_duration_predictor_twin_equals_the_oracle():
    hp = dict(O.DEFAULT_HP, n_channels=64)
    P = {k: v for k, v in O.fill_params(hp).items() if k.startswith("duration_predictor")}
    g, tl, ml, tm, mm = _case(3, 21, 50, 5)
    xs = torch.randn(3, 21, 64, generator=g)
    for inference in (False, True):
        want = O.duration_predictor(xs, P, 2, 1e-12, ~tm, inference, 1.0)
        got = R.duration_predictor(xs, P, 2, 1e-12, ~tm, inference, 1.0)
        assert torch.equal(want, got)
    P64 = {k: v.double() for k, v in P.items()}
    got64 = R.duration_predictor(xs.double(), P64, 2, 1e-12, ~tm, False, 1.0)
    want = O.duration_predictor(xs, P, 2, 1e-12, ~tm, False, 1.0)
    assert got64.dtype == torch.float64 and float((got64 - want.double()).abs().max()) <= 1e-4


def test_loss_twin_equals_the_oracle_forward(golden_dir):
    gz = np.load(os.path.join(golden_dir, "fwd_tiny.npz"))
    text, tl, speech, ml = (torch.from_numpy(gz[k]) for k in ("text", "text_lengths", "speech", "speech_lengths"))
    with torch.no_grad():
        o = O.forward(O.fill_params(), text, tl, speech, ml)
    tm, mm = R.non_pad_mask(tl, text.shape[1]), R.non_pad_mask(ml, speech.shape[1])
    mel_loss, dur_loss = R.masked_losses(o["mel_pred"], speech, o["dur_pred"], o["log_delta_e"], mm, tm)
    assert torch.equal(mel_loss, o["mel_loss"]) and torch.equal(dur_loss, o["dur_loss"])
    assert torch.equal(mel_loss + dur_loss, o["loss"])


@pytest.mark.parametrize("method1", [True, False])
def test_duration_target_twin_equals_the_oracle_forward(golden_dir, method1):
    gz = np.load(os.path.join(golden_dir, "fwd_tiny.npz"))
    text, tl, speech, ml = (torch.from_numpy(gz[k]) for k in ("text", "text_lengths", "speech", "speech_lengths"))
    hp = dict(O.DEFAULT_HP, delta_e_method_1=method1)
    with torch.no_grad():
        o = O.forward(O.fill_params(), text, tl, speech, ml, hp)
    assert int(tl.min()) < text.shape[1]                                             # (a padded token is in the batch)
    got = R.duration_target(o["e"], tl, ml, hp["duration_offset"], method1)
    assert got.dtype == torch.float32 and torch.equal(got, o["log_delta_e"])
    assert R.duration_target(o["e"].double(), tl, ml, hp["duration_offset"], method1).dtype == torch.float64


def test_twin_gradients_pass_gradcheck():
    B, T1, T2 = 2, 5, 11
    tl, ml = torch.tensor([5, 3], dtype=torch.int32), torch.tensor([11, 7], dtype=torch.int32)
    tm, mm = R.non_pad_mask(tl, T1), R.non_pad_mask(ml, T2)
    g = torch.Generator().manual_seed(3)
    p = R.index_vector(tm, torch.float64)
    gc = lambda f, x: torch.autograd.gradcheck(f, (x.clone().requires_grad_(True),), eps=1e-6, atol=1e-6, rtol=1e-5)   # noqa: E731
    s = torch.randn(B, T2, T1, generator=g, dtype=torch.float64)
    assert gc(lambda t: R.soft_index(R.attention_from_scores(t, tm), p), s)
    # strictly rising by at least 0.2 per frame: every relu is on its linear side and the maximum is unique
    sidx = (0.2 + torch.rand(B, T2, generator=g, dtype=torch.float64)).cumsum(1)
    assert gc(lambda t: R.imv_from_soft_index(t, mm, tl), sidx)
    imv = R.imv_from_soft_index(sidx, mm, tl)
    assert gc(lambda t: R.aligned_positions(t, p, mm, tm, 0.5), imv)
    e = R.aligned_positions(imv, p, mm, tm, 0.5)
    assert gc(lambda t: R.masked_ralpha(t, 0.01, mm, tm), e)
    assert gc(lambda t: R.alignment_block(t, tl, ml, 0.01, 0.5)["ralpha"], 3.0 * s)
    mel, sp = torch.randn(B, T2, 4, generator=g, dtype=torch.float64), torch.randn(B, T2, 4, generator=g, dtype=torch.float64)
    dur, lde = torch.randn(B, T1, generator=g, dtype=torch.float64), torch.randn(B, T1, generator=g, dtype=torch.float64)
    assert float((dur - lde).abs().min()) > 1e-3
    assert gc(lambda t: sum(R.masked_losses(t, sp, dur, lde, mm, tm)), mel)
    assert gc(lambda t: sum(R.masked_losses(mel, sp, t, lde, mm, tm)), dur)
    z = torch.randn(3, 8, generator=g, dtype=torch.float64)
    assert float(z.abs().min()) > 1e-3
    gm, bt = torch.randn(8, generator=g, dtype=torch.float64), torch.randn(8, generator=g, dtype=torch.float64)
    assert gc(lambda t: R.relu_layernorm(t, gm, bt, 1e-12), z)


# ---------------------------------------------------------------------------------------------------------------------
# argument checks (no device work)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from efficient_tts_amd import build as B
    from efficient_tts_amd import lib as L
    B.build(verbose=False)
    return L.load()


ESHAPE = -2
X = 0x1000            # a non-null pointer that is never dereferenced: every call below is refused before its launch


def _refused(lib, rc, *words):
    msg = lib.efts_last_error()
    assert rc == ESHAPE, (rc, msg)
    for w in words:
        assert w.encode() in msg, msg


@pytest.mark.parametrize("B,T1,T2", [(0, 8, 8), (2, 0, 8), (2, 8, 0), (-1, 8, 8), (2, -3, 8), (2, 8, -3)])
def test_alignment_bwd_refuses_non_positive_sizes(lib, B, T1, T2):
    _refused(lib, lib.efts_alpha_bwd(X, X, X, X, X, 0.01, X, X, B, T1, T2, None), "efts_alpha_bwd", "positive")
    _refused(lib, lib.efts_e_bwd(X, X, X, X, X, 0.5, X, X, B, T1, T2, None), "efts_e_bwd", "positive")
    _refused(lib, lib.efts_attn_bwd(X, max(T1, 1), X, X, X, X, X, max(T1, 1), X, 4096, B, T1, T2, max(T2, 1), None), "efts_attn_bwd", "positive")
    if B <= 0 or T2 <= 0:                       # (efts_imv_bwd has no T1)
        _refused(lib, lib.efts_imv_bwd(X, X, X, X, X, X, B, T2, None), "efts_imv_bwd", "positive")


def test_null_pointers_are_still_einval(lib):
    assert lib.efts_alpha_bwd(None, X, X, X, X, 0.01, X, X, 2, 8, 8, None) == -1 and b"null" in lib.efts_last_error()
    assert lib.efts_embed_bwd(X, None, X, 2, 8, 8, 128, 76, None) == -1 and b"null" in lib.efts_last_error()


def test_e_bwd_refuses_a_text_length_beyond_its_lds(lib):
    # 4 * T1 floats of dynamic LDS in a launch that has 64 KiB: T1 = 4096 is the last that fits
    _refused(lib, lib.efts_e_bwd(X, X, X, X, X, 0.5, X, X, 1, 4097, 64, None), "efts_e_bwd", "LDS", "4097", "4096")
    _refused(lib, lib.efts_e_bwd(X, X, X, X, X, 0.5, X, X, 1, 1 << 30, 64, None), "efts_e_bwd", "LDS")


def test_attn_bwd_refuses_short_strides(lib):
    T1, T2 = 37, 50
    ok = dict(ld=T1, ldd=T1, ldp=256, T2p=T2)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.efts_attn_bwd(X, a["ld"], X, X, X, X, X, a["ldd"], X, a["ldp"], 2, T1, T2, a["T2p"], None)
    _refused(lib, call(ld=T1 - 1), "efts_attn_bwd", "ld", "36")
    _refused(lib, call(ldd=T1 - 1), "efts_attn_bwd", "ldd", "36")
    _refused(lib, call(T2p=T2 - 1), "efts_attn_bwd", "T2p", "49")
    _refused(lib, call(ldp=128), "efts_attn_bwd", "ld_plane")          # 37 columns are two 128-byte chunks


@pytest.mark.parametrize("kw", [dict(B=0), dict(T=0), dict(Tp=7), dict(c=0), dict(c=-128), dict(nsym=0), dict(B=-2), dict(nsym=-1)])
def test_embed_bwd_refuses_bad_shapes(lib, kw):
    a = dict(dict(B=2, T=8, Tp=10, c=128, nsym=76), **kw)
    _refused(lib, lib.efts_embed_bwd(X, X, X, a["B"], a["T"], a["Tp"], a["c"], a["nsym"], None), "efts_embed_bwd", "Tp >= T")
