"""CPU: tests/train_pack_reference.py pinned -- the transposed encoders to gemm_reference's row encoder, keep_scale to the header's mixer,
the inputs of tests/test_train_pack_kernels_gpu.py to the condition of kernel_check's bound -- and the refusals the training-side
packers, efts_act_bwd and efts_wgrad_reduce answer without a device (the pointers are never dereferenced)."""
import numpy as np
import pytest
import torch

import gemm_reference as G
import train_pack_reference as R
from griffinlim_reference import _hash_u32
from kernel_check import conditioned

EINVAL, ESHAPE, EALIGN = -1, -2, -3
X = 0x1000


# ---------------------------------------------------------------------------------------------------------------------
# the encoders
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [1, 2])
@pytest.mark.parametrize("case", R.PACK_T_CASES, ids=lambda c: "-".join(map(str, c)))
def test_encode_t_is_encode_rows_of_the_shifted_transpose(case, split):
    rows, c, kpad, shift0, nshift, _, dld, dstride = case
    x = torch.randn(rows, c, generator=torch.Generator().manual_seed(rows * 100 + c))
    ld = R.kp_t(kpad, split) + dld
    stride = c * ld + dstride
    got = R.encode_t(x, rows, c, kpad, shift0, nshift, split, ld, stride)
    assert got.shape == ((nshift - 1) * stride + c * ld,)
    owned = torch.zeros_like(got, dtype=torch.bool)
    for s in range(nshift):
        xt = torch.zeros(c, kpad)                                   # explicitly: element by element
        for t in range(kpad):
            src = t + shift0 + s
            if 0 <= src < rows:
                xt[:, t] = x[src]
        want = G.encode_rows(xt, split, ld, G.CANARY)
        assert torch.equal(got[s * stride:s * stride + c * ld].view(c, ld), want)
        owned[s * stride:s * stride + c * ld] = True
    assert bool((got[~owned] == G.CANARY).all())                    # the gap between the planes
    assert bool((got.view(-1)[:c * ld].view(c, ld)[:, R.kp_t(kpad, split):] == G.CANARY).all())


@pytest.mark.parametrize("split", [1, 2])
@pytest.mark.parametrize("cout,cin,taps", R.PACK_WEIGHT_T_CASES)
def test_encode_weight_t_is_encode_weight_of_the_flipped_transpose(cout, cin, taps, split):
    w = torch.randn(cout, cin, taps, generator=torch.Generator().manual_seed(cout + cin + taps))
    ld = G.row_bytes(cout, split) + 16
    got = R.encode_weight_t(w, split, ld, G.CANARY)
    assert got.shape == (taps, cin, ld)
    assert torch.equal(got, G.encode_weight(w.flip(2).transpose(0, 1).contiguous(), split, ld, G.CANARY))
    k, ci = taps - 1, cin - 1                                       # one row by hand
    assert torch.equal(got[taps - 1 - k, ci], G.encode_rows(w[:, ci, k][None], split, ld, G.CANARY)[0])


def test_sign_words_and_sign_bits_layouts():
    pos = torch.zeros(3, 256, dtype=torch.bool)
    pos[1, 128 + 4 * 7 + 2] = True                                  # group 1, q = 7, u = 2 -> word 2, bit 7
    pos[2, 8 * 5 + 3] = True                                        # byte 5, bit 3
    w = R.sign_words(pos).numpy().view("<u4").reshape(3, 2, 4)
    assert w[1, 1, 2] == 1 << 7 and int(w.astype(np.uint64).sum()) == (1 << 7) + int(w[2].sum())
    b = R.sign_bits(pos)
    assert b.shape == (3, 32) and int(b[2, 5]) == 1 << 3 and int(b[2].sum()) == 8


# ---------------------------------------------------------------------------------------------------------------------
# the dropout mask
# ---------------------------------------------------------------------------------------------------------------------
def test_keep_scale_hash_is_the_headers_mixer():
    x = np.concatenate([np.arange(4096, dtype=np.uint64), np.array([0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 0xDEADBEEF], dtype=np.uint64)])
    assert np.array_equal(R.hash_u32(x).astype(np.uint64), _hash_u32(x))
    assert int(R.hash_u32(np.uint32(0))) == 0


@pytest.mark.parametrize("p", R.DROP_PS)
@pytest.mark.parametrize("seed", R.DROP_SEEDS)
def test_keep_scale_share_and_values(p, seed):
    n = 1 << 16
    ks = R.keep_scale(seed, np.arange(n), p)
    thresh, inv_keep = R.drop_params(p)
    assert ks.dtype == np.float32 and inv_keep.dtype == np.float32
    assert int(thresh) == int(float(np.float32(p)) * 2.0 ** 32)
    assert inv_keep == np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    assert set(np.unique(ks)) == {np.float32(0.0), inv_keep}
    kept = float((ks != 0).mean())
    sigma = (p * (1 - p) / n) ** 0.5
    assert abs(kept - (1 - p)) <= 4 * sigma, (kept, 1 - p, sigma)
    # element by element against the shared mixer: keep iff hash(idx ^ hash(seed)) >= thresh
    seed_h = _hash_u32(np.array([seed], dtype=np.uint64))[0]
    h = _hash_u32(np.arange(n, dtype=np.uint64) ^ seed_h)
    assert np.array_equal(ks != 0, h >= np.uint64(int(thresh)))


# ---------------------------------------------------------------------------------------------------------------------
# the bound's condition on the inputs of the GPU file: FACTOR * e32 <= COND for every reduction
# ---------------------------------------------------------------------------------------------------------------------
def _assert_conditioned(cases):
    n = 0
    for name, ref64, ref32 in cases:
        ok, e32 = conditioned(ref64, ref32)
        assert ok, f"{name}: inputs too ill-conditioned for the bound to mean anything (e32 = {e32:.3e})"
        n += 1
    return n


def test_act_bwd_column_sums_are_conditioned():
    assert _assert_conditioned(R.act_reduction_cases()) > 100


def test_wgrad_reduce_cases_are_conditioned():
    assert _assert_conditioned(R.wgrad_reduction_cases()) == 3 * len(R.WGRAD_CASES)


def test_weight_norm_folds_are_conditioned():
    assert _assert_conditioned(R.fold_reduction_cases()) == 5 * 7


def test_act_inputs_keep_their_distance_from_zero():
    for rows, c in R.ACT_SHAPES:
        for mode in (1, 2, 3):
            i = R.act_inputs(rows, c, mode, True)
            d = (i.y - i.x) if mode == 1 else i.y
            assert float(d.abs().min()) >= 1e-3
    for mode in (1, 2, 3):
        i = R.act_inputs(*R.ACT_ZERO_SHAPE, mode, True, True)
        d = ((i.y - i.x) if mode == 1 else i.y).view(-1)
        assert bool((d[i.planted[16:48]] == 0).all())
        r = R.act_reference(*R.ACT_ZERO_SHAPE, mode, True, True)
        rm = i.rm[i.planted[16:48] // R.ACT_ZERO_SHAPE[1]]
        neg = 0.0 if mode == 2 else np.float32(R.ACT_SLOPE)
        assert torch.equal(r.dz.view(-1)[i.planted[16:48]], i.g.view(-1)[i.planted[16:48]] * (neg * rm))     # the slope / 0 branch


def test_act_bwd_ref_matches_autograd_of_the_activations():
    """mode 1 / 2 / 3 against torch autograd of x + leaky(z), relu(z), leaky(z) in float64"""
    rows, c = 65, 132
    for mode in (1, 2, 3):
        i = R.act_inputs(rows, c, mode, True)
        r = R.act_reference(rows, c, mode, True)
        z = ((i.y - i.x) if mode == 1 else i.y).double().requires_grad_(True)      # the sign of z is the sign of these
        f = torch.relu(z) if mode == 2 else torch.nn.functional.leaky_relu(z, float(np.float32(R.ACT_SLOPE)))
        (gz,) = torch.autograd.grad((f * (i.g.double() * i.rm.double()[:, None])).sum(), z)
        assert float((gz - r.dz.double()).abs().max()) <= 1e-6
        assert float((gz.sum(0) - r.col64).abs().max()) <= 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# refusals (no device work)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from efficient_tts_amd import build as B
    from efficient_tts_amd import lib as L
    B.build(verbose=False)
    return L.load()


def test_pack_t_refusals(lib):
    ok = dict(ldx=80, ld=256, stride=80 * 256, split=1, rows=63, c=80, shift0=-2, nshift=5, kpad=64)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.efts_pack_t(X, a["ldx"], X, a["ld"], a["stride"], a["split"], a["rows"], a["c"], a["shift0"], a["nshift"], a["kpad"], None)

    assert call(kpad=96) == ESHAPE and b"kpad" in lib.efts_last_error()
    for nshift in (0, 12):
        assert call(nshift=nshift) == ESHAPE and b"nshift" in lib.efts_last_error()
    assert call(ld=127) == ESHAPE and b"ld_plane" in lib.efts_last_error()                 # 64 bf16 need 128 bytes
    assert call(split=2, ld=255) == ESHAPE and b"ld_plane" in lib.efts_last_error()        # 64 hi/lo pairs need 256


def test_act_bwd_refusals(lib):
    from efficient_tts_amd import lib as L

    def call(mode, c, dbias=None, y=X, x=X):
        return lib.efts_act_bwd(X, y, x, None, 0.1, mode, X, None, 0, 1, dbias, 8, c, None)

    assert call(0, 30) == EINVAL and b"efts_act_bwd" in lib.efts_last_error()              # c % 4 != 0
    assert call(6, 128) == EINVAL
    assert call(4, 192) == EINVAL                                                          # mode 4: c % 128 != 0
    assert call(5, 132) == EINVAL                                                          # mode 5: c % 8 != 0
    assert call(0 | L.ACT_BWD_BIAS_PARTS, 128, dbias=None) == EINVAL                       # BIAS_PARTS without dbias
    assert lib.efts_act_bwd_dropout(X, None, None, None, 0.1, 0, X, None, 0, 1, None, 8, 128, 1.0, 7, None) == EINVAL
    assert b"drop_p" in lib.efts_last_error()
    # a plane whose rows can not hold Kp(c) values (the kernel writes the K padding too)
    assert lib.efts_act_bwd(X, None, None, None, 0.1, 0, None, X, 255, 1, None, 8, 80, None) == ESHAPE      # Kp = 128 bf16 = 256 bytes
    assert b"ld_plane" in lib.efts_last_error()
    assert lib.efts_act_bwd(X, None, None, None, 0.1, 0, None, X, 383, 2, None, 8, 80, None) == ESHAPE      # Kp = 96 pairs = 384 bytes


def test_wgrad_reduce_refuses_rows_beyond_its_lds(lib):
    assert lib.efts_wgrad_reduce(X, 3, None, None, X, None, 8, 3001, 5, None) == ESHAPE    # 3001 * 5 * 4 = 60020 > 60000
    assert b"LDS" in lib.efts_last_error()
    assert lib.efts_wgrad_reduce(X, 3, None, X, X, X, 8, 64, 5, None) == EINVAL            # g without v


@pytest.mark.parametrize("split", [1, 2])
def test_weight_packers_refuse_a_bad_row_stride(lib, split):
    cout, cin, taps = 80, 130, 3
    need, need_t = G.row_bytes(cin, split), G.row_bytes(cout, split)
    for ldb in (need_t - 16, need_t + 8):                                                  # too small; not 16-byte aligned
        assert lib.efts_pack_weight_t(X, X, ldb, cout, cin, taps, split, None) == EALIGN
        assert b"ldb" in lib.efts_last_error()
    for ldb in (need - 16, need + 8):
        assert lib.efts_pack_weights_grouped(X, 1, None, ldb, need_t, cout, cin, taps, split, 1, None) == EALIGN
        assert b"ldb" in lib.efts_last_error()
    for ldb_t in (need_t - 16, need_t + 8):
        assert lib.efts_pack_weights_grouped(X, 1, None, need, ldb_t, cout, cin, taps, split, 1, None) == EALIGN
        assert b"ldb_t" in lib.efts_last_error()
