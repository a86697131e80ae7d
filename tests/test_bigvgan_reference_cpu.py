"""CPU: the reference `efts_snake_aa` is tested against (tests/bigvgan_reference.py)  --  the anti-aliasing filter and the definition of the
activation that include/efts_abi.h states, against the torch-op composition.  No launch."""
import os

import pytest
import torch

import bigvgan_reference as BR

LENGTHS = (1, 2, 3, 5, 6, 7, 11, 12, 13, 40)


def test_filter_is_the_pinned_kaiser_sinc():
    f = BR.aa_filter()
    assert f.dtype == torch.float64 and f.shape == (12,)
    for k, want in enumerate(BR.PINNED):
        assert abs(float(f[k]) - want) <= 1e-15 and abs(float(f[11 - k]) - want) <= 1e-15
    assert abs(float(f.sum()) - 1.0) <= 1e-15
    assert torch.equal(f.float(), f.float().flip(0))                 # symmetric to the bit once rounded: the kernel holds six numbers
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "efts_abi.h")).read()
    for want in BR.PINNED:                                           # the header states the same six numbers
        assert repr(abs(want)) in hdr


@pytest.mark.parametrize("L", LENGTHS)
def test_composition_equals_the_direct_double_clamp_form(L):
    g = torch.Generator().manual_seed(L)
    x = 2 * torch.randn(3, L, generator=g, dtype=torch.float64)
    a, inv_b = torch.exp(0.5 * torch.randn(3, generator=g)), torch.exp(0.5 * torch.randn(3, generator=g))
    got = BR.activation1d(x[None], a.double(), inv_b.double())[0]
    want = BR.activation1d_direct(x, a, inv_b)
    assert float((got - want).abs().max()) <= 1e-14


def test_constant_input_gives_the_pointwise_snake():
    """Replicate padding makes a constant sequence constant at the 2x rate and behind the low-pass.  The twelve taps are rounded to fp32
    (2^-24 each, sum |f| = 1.33), so each half filter sums to 0.5 and the whole to 1 within 8e-8 only; through 2 * |c| <= 3 and the slope of
    the activation, at most 1 + 2 a inv_b <= 3.4 here, that is below 1e-6."""
    for L in (1, 4, 17):
        for c in (-1.5, 0.0, 0.7):
            a, inv_b = torch.tensor([1.3, 0.6], dtype=torch.float64), torch.tensor([0.8, 2.0], dtype=torch.float64)
            y = BR.activation1d(torch.full((1, 2, L), c, dtype=torch.float64), a, inv_b)
            want = (c + inv_b * torch.sin(a * c) ** 2).view(1, 2, 1).expand(1, 2, L)
            assert float((y - want).abs().max()) <= 1e-6
