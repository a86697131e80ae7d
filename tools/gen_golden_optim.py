#!/usr/bin/env python3
"""Golden fixture for the fused RAdam, produced by the REFERENCE's own optimizer (build container only):

    python tools/gen_golden_optim.py /root/reference

loads nntts/optimizers/radam.py by path (nothing else of the reference is imported) and runs 8 steps in fp32 on seeded parameters and
gradients, n = 1031, at three settings: the recipe's Adam hyper-parameters (betas (0.9, 0.99), eps 1e-9, weight decay 1e-5), the
class defaults, and the recipe's with weight decay 1e-2 -- the one setting whose decay factor 1 - lr * wd fp32 can tell from 1 (at 1e-5 it
rounds to 1.0f, the defaults have none).  Eight steps because N_sma is 4.96 / 4.996 at step 5 and 5.94 / 5.99 at step 6 for beta2 0.99 / 0.999: steps 1-5 take
the unrectified branch, 6-8 the rectified one.  Writes tests/golden/radam_small.npz -- inputs, per-step parameters, final moments;
only data is stored."""
import importlib.util
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, STEPS = 1031, 8
SETTINGS = dict(recipe=dict(lr=1e-3, betas=(0.9, 0.99), eps=1e-9, weight_decay=1e-5),
                default=dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0),
                decay=dict(lr=1e-3, betas=(0.9, 0.99), eps=1e-9, weight_decay=1e-2))


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("EFTS_REFERENCE", "")
    spec = importlib.util.spec_from_file_location("ref_radam", os.path.join(ref, "nntts", "optimizers", "radam.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    warnings.simplefilter("ignore")                                  # (the file uses add_(Number, Tensor), deprecated in torch)
    gen = torch.Generator().manual_seed(1031)
    p0 = torch.randn(N, generator=gen)
    grads = torch.randn(STEPS, N, generator=gen)                     # N(0, 1): nowhere near eps, where m / sqrt(v) is ill-conditioned
    out = dict(p0=p0.numpy(), grads=grads.numpy(), names=np.array(list(SETTINGS)))
    for name, kw in SETTINGS.items():
        p = torch.nn.Parameter(p0.clone())
        opt = mod.RAdam([p], **kw)
        traj = []
        for t in range(STEPS):
            p.grad = grads[t].clone()
            opt.step()
            traj.append(p.detach().clone().numpy())
        st = opt.state[p]
        assert st["step"] == STEPS
        out.update({f"{name}:hyper": np.array([kw["lr"], *kw["betas"], kw["eps"], kw["weight_decay"]], np.float64),
                    f"{name}:params": np.stack(traj), f"{name}:exp_avg": st["exp_avg"].numpy(), f"{name}:exp_avg_sq": st["exp_avg_sq"].numpy()})
    path = os.path.join(ROOT, "tests", "golden", "radam_small.npz")
    np.savez(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
