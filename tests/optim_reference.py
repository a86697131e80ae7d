"""float64 restatement of the update rules behind efts_optim_step (include/efts_abi.h), for the optimizer tests: the clip of
`clip_grad_norm_` folded into the kernel, torch.optim.Adam, torch.optim.AdamW and the reference recipe's RAdam.  numpy only, written
from the formulas; tests/test_optim_cpu.py holds it against torch's own optimizers and against a run recorded from the reference's RAdam
(tests/golden/radam_small.npz)."""
import math

import numpy as np

ADAM, ADAMW, RADAM = 0, 1, 2


def clip_coef(g, max_norm, gscale=1.0):
    """the factor in front of the raw gradient: gscale * min(1, max_norm / (||gscale * g|| + 1e-6)); max_norm <= 0: no clip"""
    if max_norm <= 0:
        return float(gscale)
    nrm = math.sqrt(float(np.sum(np.asarray(g, np.float64) ** 2))) * gscale
    return float(gscale) * min(1.0, max_norm / (nrm + 1e-6))


def radam_rectification(t, beta2):
    """(N_sma, rectified, step size without 1 / (1 - beta1^t)) of step t"""
    b2t = beta2 ** t
    nmax = 2.0 / (1.0 - beta2) - 1.0
    nsma = nmax - 2.0 * t * b2t / (1.0 - b2t)
    if nsma >= 5:
        return nsma, True, math.sqrt((1.0 - b2t) * (nsma - 4.0) / (nmax - 4.0) * (nsma - 2.0) / nsma * nmax / (nmax - 2.0))
    return nsma, False, 1.0


def step(algo, p, g, m, v, vmax, t, lr, betas, eps, wd, amsgrad=False, max_norm=0.0, gscale=1.0):
    """one update of step number t >= 1 on float64 arrays; returns new (p, m, v, vmax) -- vmax passes through untouched without amsgrad"""
    b1, b2 = betas
    p, m, v = (np.asarray(x, np.float64) for x in (p, m, v))
    gg = clip_coef(g, max_norm, gscale) * np.asarray(g, np.float64)
    if algo == ADAM:
        gg = gg + wd * p
    elif algo == ADAMW:
        p = p * (1.0 - lr * wd)
    m = b1 * m + (1.0 - b1) * gg
    v = b2 * v + (1.0 - b2) * gg * gg
    bc1 = 1.0 - b1 ** t
    if algo == RADAM:
        assert not amsgrad
        _, rect, s = radam_rectification(t, b2)
        if wd != 0:
            p = p - wd * lr * p
        p = p - lr * s / bc1 * m / (np.sqrt(v) + eps) if rect else p - lr / bc1 * m
        return p, m, v, vmax
    vh = v
    if amsgrad:
        vmax = np.maximum(np.asarray(vmax, np.float64), v)
        vh = vmax
    p = p - (lr / bc1) * m / (np.sqrt(vh) / math.sqrt(1.0 - b2 ** t) + eps)
    return p, m, v, vmax


def run(algo, p0, grads, lr, betas, eps, wd, amsgrad=False, max_norm=0.0, gscale=1.0):
    """len(grads) steps from zero moments; returns (per-step parameters [steps][n], m, v, vmax)"""
    p = np.asarray(p0, np.float64)
    m, v = np.zeros_like(p), np.zeros_like(p)
    vmax = np.zeros_like(p) if amsgrad else None
    traj = []
    for t, g in enumerate(grads, 1):
        p, m, v, vmax = step(algo, p, g, m, v, vmax, t, lr, betas, eps, wd, amsgrad, max_norm, gscale)
        traj.append(p)
    return np.stack(traj), m, v, vmax


# ---- what the optimizer tests share besides the rules: the error metric, and the stock torch optimizers run on the CPU
def relerr(got, ref):
    """max |got - ref| / max |ref| (the metric of every bound in the optimizer tests)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max()) / (float(np.abs(ref).max()) + 1e-300)


def torch_run(algo, p0, grads, lr, betas, eps, wd, amsgrad=False, max_norm=0.0, dtype="float64"):
    """torch.optim.Adam / AdamW (+ clip_grad_norm_) on the CPU in `dtype`; returns what `run` returns"""
    import torch
    dt = getattr(torch, dtype)
    p = torch.nn.Parameter(torch.tensor(np.array(p0)).to(dt))
    cls = {ADAM: torch.optim.Adam, ADAMW: torch.optim.AdamW}[algo]
    opt = cls([p], lr=lr, betas=betas, eps=eps, weight_decay=wd, amsgrad=amsgrad, foreach=False)
    traj = []
    for g in grads:
        p.grad = torch.tensor(np.array(g)).to(dt)
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_([p], max_norm)
        opt.step()
        traj.append(p.detach().clone().numpy())
    st = opt.state[p]
    return np.stack(traj), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy(), st["max_exp_avg_sq"].numpy() if amsgrad else None


def fp32_gap(algo, p0, grads, hyper, amsgrad=False, max_norm=0.0, ref=None):
    """(parameters, exp_avg, exp_avg_sq[, max_exp_avg_sq]) relerr of torch's own fp32 CPU optimizer against the float64 restatement (`ref`,
    where the caller has run it already): what fp32 arithmetic costs on these inputs, the unit of the device bounds"""
    if ref is None:
        ref = run(algo, p0, grads, *hyper, amsgrad=amsgrad, max_norm=max_norm)
    got = torch_run(algo, np.asarray(p0, np.float32), np.asarray(grads, np.float32), *hyper, amsgrad=amsgrad, max_norm=max_norm, dtype="float32")
    return [relerr(a, b) for a, b in zip(got, ref) if b is not None]
