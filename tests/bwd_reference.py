"""Dtype-generic twins of the oracle functions the training-side kernels differentiate  --  TEST INFRASTRUCTURE.

``oracle/efts_oracle.py`` builds float32 ``arange``s, so its functions can not serve as a float64 reference.  Every function
here is a plain transcription of the oracle function of the same name in which the working dtype follows the input: evaluated
in float32 it performs the very operations of the oracle (``tests/test_bwd_reference_cpu.py`` asserts ``torch.equal``), evaluated
in float64 it is the reference of ``tests/test_bwd_kernels_gpu.py`` (value and, through torch autograd, gradient).

Two oracle functions are cut at the tensor a kernel starts from, so that a stage can be differentiated alone:
``scaled_dot_attention`` = ``attention_from_scores`` after the scaled product, ``imv_generator`` = ``imv_from_soft_index`` after
``soft_index``.  Plain module, no GPU, no library.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F


def non_pad_mask(lengths: torch.Tensor, maxlen: int) -> torch.Tensor:
    return torch.arange(maxlen)[None, :] < lengths.to(torch.int64)[:, None]


def index_vector(text_mask: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """p[b,i] = i * text_mask[b,i]"""
    return torch.arange(text_mask.shape[1], dtype=dtype)[None, :] * text_mask


def attention_from_scores(s: torch.Tensor, key_mask: torch.Tensor) -> torch.Tensor:
    """s[B,T2,T1] (already scaled) -> alpha[B,T1,T2]: softmax over T1, padded keys -> 0"""
    dead = ~key_mask[:, None, :]
    a = torch.softmax(s.masked_fill(dead, -float("inf")), dim=-1).masked_fill(dead, 0.0)
    return a.transpose(1, 2)


def scaled_dot_attention(q: torch.Tensor, k: torch.Tensor, key_mask: torch.Tensor) -> torch.Tensor:
    s = torch.bmm(q, k.transpose(1, 2)) / math.sqrt(float(k.shape[-1]))
    return attention_from_scores(s, key_mask)


def soft_index(alpha: torch.Tensor, p: torch.Tensor) -> torch.Tensor:
    return torch.einsum("bij,bi->bj", alpha, p)


def imv_from_soft_index(soft_idx: torch.Tensor, mel_mask: torch.Tensor, text_lengths: torch.Tensor) -> torch.Tensor:
    d = torch.relu(soft_idx[:, 1:] - soft_idx[:, :-1])
    d = torch.cat([torch.zeros_like(soft_idx[:, :1]), d], dim=1)
    pi = torch.cumsum(d, dim=1) * mel_mask.to(soft_idx.dtype)
    top = pi.max(dim=1).values.clamp(min=1e-8)
    return pi / top[:, None] * (text_lengths.to(soft_idx.dtype)[:, None] - 1.0)


def imv_generator(alpha: torch.Tensor, p: torch.Tensor, mel_mask: torch.Tensor, text_lengths: torch.Tensor) -> torch.Tensor:
    return imv_from_soft_index(soft_index(alpha, p), mel_mask, text_lengths)


def aligned_positions(pi: torch.Tensor, p: torch.Tensor, mel_mask: torch.Tensor, text_mask: torch.Tensor, sigma_e: float) -> torch.Tensor:
    en = -sigma_e * (pi[:, None, :] - p[:, :, None]) ** 2
    en = en.masked_fill(~mel_mask[:, None, :], -float("inf"))
    beta = torch.softmax(en, dim=2)
    q = torch.arange(mel_mask.shape[1], dtype=pi.dtype)[None, :] * mel_mask.to(pi.dtype)
    return torch.einsum("bij,bj->bi", beta, q) * text_mask.to(pi.dtype)


def reconstruct_alignment(e: torch.Tensor, sigma: float, mel_mask: torch.Tensor, text_mask: torch.Tensor) -> torch.Tensor:
    """the training form (both masks given); callers apply masked_fill(~both, 0) as the oracle's forward does"""
    t2 = mel_mask.shape[1]
    q = torch.arange(t2, dtype=e.dtype)[None, :].expand(e.shape[0], t2)
    q = q * mel_mask.to(e.dtype)
    en = -sigma * (q[:, None, :] - e[:, :, None]) ** 2
    en = en.masked_fill(~text_mask[:, :, None], -float("inf"))
    return torch.softmax(en, dim=1)


def masked_ralpha(e, sigma, mel_mask, text_mask):
    """alpha' as the forward keeps it (efts_oracle.forward, `ralpha`): zero outside text x mel"""
    both = text_mask[:, :, None] & mel_mask[:, None, :]
    return reconstruct_alignment(e, sigma, mel_mask, text_mask).masked_fill(~both, 0.0)


def duration_target(e, text_lengths, mel_lengths, offset, method1):
    """log_delta_e of efts_oracle.forward (:307-314): method 1 e_i - e_{i-1} with e_{-1} = 0, otherwise e_{i+1} - e_i with
    e_{text_len} = mel_len; log(. + offset), 0 at padded tokens"""
    if method1:
        delta_e = torch.cat([e[:, :1], e[:, 1:] - e[:, :-1]], dim=1)
    else:
        ee = torch.cat([e, torch.zeros(e.shape[0], 1, dtype=e.dtype)], dim=1)
        for i in range(e.shape[0]):
            ee[i, int(text_lengths[i])] = float(mel_lengths[i])
        delta_e = ee[:, 1:] - ee[:, :-1]
    return torch.log(delta_e + offset).masked_fill(~non_pad_mask(text_lengths, e.shape[1]), 0.0)


def masked_losses(mel_pred, speech, dur_pred, log_delta_e, mel_mask, text_mask):
    """FastSpeechLoss(use_masking=True) as efts_oracle.forward takes it: (mel_loss, dur_loss)"""
    n_mel = mel_mask.sum() * speech.shape[2]
    mel_loss = (((mel_pred - speech) ** 2) * mel_mask[:, :, None]).sum() / n_mel
    dur_loss = ((dur_pred - log_delta_e).abs() * text_mask).sum() / text_mask.sum()
    return mel_loss, dur_loss


def relu_layernorm(z, gamma, beta, eps):
    """one duration-predictor layer behind its conv: LayerNorm over channels of relu(z); z [..., C]"""
    return F.layer_norm(F.relu(z), (z.shape[-1],), gamma, beta, eps)


def duration_predictor(xs, P, n_layers, eps, pad_mask, inference, offset):
    h = xs.transpose(1, 2)
    for i in range(n_layers):
        p = f"duration_predictor.conv.{i}."
        z = F.conv1d(h, P[p + "0.weight"], P[p + "0.bias"], padding=1)
        h = relu_layernorm(z.transpose(1, 2), P[p + "2.weight"], P[p + "2.bias"], eps).transpose(1, 2)
    out = F.linear(h.transpose(1, 2), P["duration_predictor.linear.weight"], P["duration_predictor.linear.bias"]).squeeze(-1)
    if inference:
        out = torch.clamp(out.exp() - offset, min=0)
    if pad_mask is not None:
        out = out.masked_fill(pad_mask, 0.0)
    return out


def alignment_block(scores, text_lengths, mel_lengths, sigma, sigma_e):
    """scores[B,T2,T1] -> every stage of the alignment block in the dtype of `scores` (efts_oracle.forward :167-186)"""
    B, T2, T1 = scores.shape
    text_mask, mel_mask = non_pad_mask(text_lengths, T1), non_pad_mask(mel_lengths, T2)
    both = text_mask[:, :, None] & mel_mask[:, None, :]
    alpha = attention_from_scores(scores, text_mask).masked_fill(~both, 0.0)
    p = index_vector(text_mask, scores.dtype)
    sidx = soft_index(alpha, p)
    imv = imv_from_soft_index(sidx, mel_mask, text_lengths)
    e = aligned_positions(imv, p, mel_mask, text_mask, sigma_e)
    ralpha = masked_ralpha(e, sigma, mel_mask, text_mask)
    return dict(alpha=alpha, soft_idx=sidx, imv=imv, e=e, ralpha=ralpha, text_mask=text_mask, mel_mask=mel_mask, p=p)


# ---------------------------------------------------------------------------------------------------------------------
# inputs of the kernel tests (deterministic, CPU)
# ---------------------------------------------------------------------------------------------------------------------
def ragged_lengths(B, T, g, first_full=True, last=None):
    """item 0 spans the padded length (a real batch is padded to its longest item), the others are shorter; `last` pins the last one"""
    ln = torch.randint(max(1, T // 3), T + 1, (B,), generator=g)
    if first_full:
        ln[0] = T
    if last is not None and B > 1:
        ln[B - 1] = min(last, T)
    return ln.to(torch.int32)


def rising_soft_index(tl, ml, T2, g, noise=0.3):
    """float32 [B,T2]: rises from 0 to text_len - 1 over the item's frames and on beyond them, with noise of about `noise`"""
    j = torch.arange(T2, dtype=torch.float64)[None, :]
    ramp = j / (ml.double()[:, None] - 1.0).clamp(min=1.0) * (tl.double()[:, None] - 1.0)
    return (ramp + noise * torch.randn(len(tl), T2, generator=g, dtype=torch.float64)).float()


def scores_for(tl, ml, T1, T2, g, ld=None, noise=0.3, sharp=0.5):
    """float32 scores [B,T2,ld] whose soft index is about rising_soft_index(): -sharp (i - c_j)^2 plus noise of a few tenths"""
    c = rising_soft_index(tl, ml, T2, g, noise).double()
    i = torch.arange(T1, dtype=torch.float64)[None, None, :]
    s = -sharp * (i - c[:, :, None]) ** 2 + 0.3 * torch.randn(len(tl), T2, T1, generator=g, dtype=torch.float64)
    out = torch.full((len(tl), T2, ld or T1), 7.0, dtype=torch.float32)           # columns >= T1 are never read
    out[:, :, :T1] = s.float()
    return out
