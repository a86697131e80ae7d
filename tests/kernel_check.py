"""The metric and the bound of the single-kernel tests  --  TEST INFRASTRUCTURE, one definition for
tests/test_bwd_kernels_gpu.py, tests/test_fwd_kernels_gpu.py and tests/test_act_kernels_gpu.py.

`_rel` = max |got - ref| / max |ref| over the tensor.  For every case the same transcription is also evaluated in float32 torch on
the CPU; its error against float64 is `e32`, and the kernel must be within max(FACTOR * e32, FLOOR).  The bound can not grow until
it hides an error: FACTOR * e32 <= COND is asserted for every case (tests/test_fwd_reference_cpu.py asserts it for the forward and
activation cases without a device).  Plain module: importing it needs neither a GPU nor the library.
"""
import torch

FACTOR, FLOOR, COND = 8.0, 2e-6, 2e-4


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def load_lib():
    """the body of the `lib` fixture of the GPU files"""
    from efficient_tts_amd import lib as L
    L.require_device()
    return L.load()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _call(name, rc):
    from efficient_tts_amd import lib as L
    L.check(rc, name)


def _rel(a, b):
    return float((a - b).abs().max()) / (float(b.abs().max()) + 1e-12)


def conditioned(ref64, ref32):
    """(FACTOR * e32 <= COND, e32): the condition `_check` asserts, from the two CPU transcriptions alone"""
    e32 = _rel(ref32.detach().double().reshape(ref64.shape), ref64)
    return FACTOR * e32 <= COND, e32


def _check(kernel, case, got, ref64, ref32, chain=False, extra=0.0):
    """got (device or host tensor) against the float64 reference, bounded by the float32 transcription's own error.
    chain: the bound is min(max(8 * e32, 2e-6), 2e-4) instead of the condition on e32 (see test_alignment_backward_chain_vs_fp64)
    extra: the resolution of the storage format `got` was decoded from (2^-16 for a bf16x3 plane, 2^-8 for a bf16 one), added to the bound"""
    got = got.detach().cpu().double().reshape(ref64.shape)
    e32 = _rel(ref32.detach().double().reshape(ref64.shape), ref64)
    err = _rel(got, ref64)
    ratio = err / e32 if e32 > 0 else float("inf") if err > 0 else 0.0
    print(f"RATIO {kernel} {case} err={err:.3e} e32={e32:.3e} ratio={ratio:.2f}")
    assert torch.isfinite(got).all()
    if not chain:
        assert FACTOR * e32 <= COND, f"{kernel} {case}: inputs too ill-conditioned for the bound to mean anything (e32 = {e32:.3e})"
    assert err <= min(max(FACTOR * e32, FLOOR), COND) + extra, f"{kernel} {case}: error {err:.3e} vs float64, float32 transcription {e32:.3e}"


def unpack_plane(pl, B, Tp, T, kp, split, parts=False):
    """rows (b * Tp + j), j < T, of an operand plane [B * Tp][ld bytes] -> float32 [B, T, kp].  Format 1: kp bf16; format 2: every
    128-byte chunk holds 32 hi then 32 lo bf16, the value is hi + lo (tests/test_align_gpu.py, test_pack_vt_layout_both_kernels);
    format 3: kp float32 (tests/test_gpu_fp32.py).
    parts: (hi, lo) instead of the value -- the two numbers a format-2 contraction multiplies (lo is zero for formats 1 and 3)"""
    raw = pl.cpu()
    if split == 3:
        v = raw.view(torch.float32).view(B, Tp, -1)[:, :T, :kp].clone()
        return (v, torch.zeros_like(v)) if parts else v
    if split == 1:
        v = raw.view(torch.bfloat16).view(B, Tp, -1)[:, :T, :kp].float()
        return (v, torch.zeros_like(v)) if parts else v
    nchunk = kp // 32
    w = raw.view(torch.bfloat16).view(B, Tp, -1)[:, :T, :nchunk * 64].reshape(B, T, nchunk, 2, 32).float()
    if parts:
        return w[:, :, :, 0].reshape(B, T, kp), w[:, :, :, 1].reshape(B, T, kp)
    return (w[:, :, :, 0] + w[:, :, :, 1]).reshape(B, T, kp)
