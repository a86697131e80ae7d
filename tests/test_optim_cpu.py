"""CPU: the optimizer family behind the registry (efficient_tts_amd/optimizers.py: Adam, AdamW, RAdam) -- everything that needs no device.

The float64 restatement of the rules (tests/optim_reference.py), which tests/test_optim_gpu.py holds the kernel against, is itself held
against torch's own Adam / AdamW and against a run recorded from the reference's RAdam; the host half of the C ABI (efts_optim_hyper,
argument errors, struct layout) and the registry are checked as far as a CPU reaches."""
import ctypes as C
import importlib.util
import math
import os
import struct

import numpy as np
import pytest

import optim_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECIPE = (1e-3, (0.9, 0.99), 1e-9, 1e-5)               # the recipe's Adam hyper-parameters (lr, betas, eps, weight_decay)
HYPER = {R.ADAM: RECIPE, R.ADAMW: (1e-3, (0.9, 0.999), 1e-8, 1e-2)}

# The RAdam fixture is fp32, the restatement float64.  The unit of their distance is what fp32 costs torch's OWN Adam on the same inputs
# (optim_reference.fp32_gap, measured at run time), times 4 for the different order of operations of the two rules.
# Measured on the 1031-element fixture inputs, recipe hyper-parameters, 8 steps (parameters, exp_avg, exp_avg_sq):
#   torch Adam fp32 vs float64        1.23e-07  7.17e-08  1.69e-07
#   fixture "recipe" vs restatement   1.33e-07  1.78e-07  1.08e-07
#   fixture "default" vs restatement  1.69e-07  1.78e-07  1.72e-07
#   fixture "decay" vs restatement    3.04e-07  1.78e-07  1.08e-07   (one more rounding per step and element: p * (1 - lr * wd))
FIXTURE_GAP_FACTOR = 4.0


@pytest.fixture(scope="module")
def radam(golden_dir):
    return np.load(os.path.join(golden_dir, "radam_small.npz"))


@pytest.fixture(scope="module")
def lib():
    from efficient_tts_amd import build as B, lib as L
    B.build(verbose=False)
    return L.load()


@pytest.mark.parametrize("max_norm", [0.0, 1.0])
@pytest.mark.parametrize("amsgrad", [False, True])
@pytest.mark.parametrize("algo", [R.ADAM, R.ADAMW])
def test_restatement_equals_torch_in_float64(radam, algo, amsgrad, max_norm):
    """8 steps of torch.optim.Adam / AdamW (+ clip_grad_norm_) in float64 on the CPU: parameters of every step and the moments, to 1e-12"""
    p0, grads = radam["p0"].astype(np.float64), radam["grads"].astype(np.float64)
    ref = R.torch_run(algo, p0, grads, *HYPER[algo], amsgrad=amsgrad, max_norm=max_norm)
    got = R.run(algo, p0, grads, *HYPER[algo], amsgrad=amsgrad, max_norm=max_norm)
    assert (got[3] is None) == (not amsgrad)
    for a, b in zip(got, ref):
        if b is not None:
            assert R.relerr(a, b) <= 1e-12


def test_restatement_equals_the_reference_radam_run(radam):
    """the recorded fp32 run of the reference's RAdam (tools/gen_golden_optim.py) at every setting, across the rectification switch"""
    p0, grads = radam["p0"], radam["grads"]
    assert grads.shape == (8, 1031) and float(np.abs(grads).min()) > 1e-6          # nowhere near eps
    unit = R.fp32_gap(R.ADAM, p0, grads, RECIPE)
    assert all(5e-9 < u < 1e-6 for u in unit), unit                               # (an fp32 rounding scale, not a degenerate 0)
    for name in radam["names"]:
        h = radam[f"{name}:hyper"]
        hyper = (float(h[0]), (float(h[1]), float(h[2])), float(h[3]), float(h[4]))
        branches = [R.radam_rectification(t, hyper[1][1])[1] for t in range(1, 9)]
        assert branches == [False] * 5 + [True] * 3                               # both branches occur: 1-5 plain, 6-8 rectified
        traj, m, v, _ = R.run(R.RADAM, p0, grads, *hyper)
        err = [R.relerr(radam[f"{name}:params"], traj), R.relerr(radam[f"{name}:exp_avg"], m), R.relerr(radam[f"{name}:exp_avg_sq"], v)]
        print(name, "fixture vs restatement", err, "unit", unit)
        for e, u in zip(err, unit):
            assert e <= FIXTURE_GAP_FACTOR * u, (name, err, unit)
        # the switch is visible: the rectified step 6 is far shorter than the plain step 5 (step size 0.042 against 2.44 per unit of m)
        d5, d6 = np.abs(traj[4] - traj[3]).max(), np.abs(traj[5] - traj[4]).max()
        assert d6 < 0.2 * d5
    # "decay" is the setting whose decoupled decay is visible at the bound: 8 steps of p -= wd * lr * p at wd 1e-2 shrink p by 8e-5,
    # a restatement without it would miss the recorded parameters by a hundred times the bound
    assert set(radam["names"]) == {"recipe", "default", "decay"} and radam["decay:hyper"][4] == 1e-2
    h = radam["decay:hyper"]
    undecayed = R.run(R.RADAM, p0, grads, float(h[0]), (float(h[1]), float(h[2])), float(h[3]), 0.0)[0]
    assert R.relerr(radam["decay:params"], undecayed) > 100 * FIXTURE_GAP_FACTOR * unit[0]


def test_registry_has_the_three_names():
    from efficient_tts_amd import optim, optimizers
    assert (optimizers.Adam, optimizers.AdamW, optimizers.RAdam) == (optim.EftsAdam, optim.EftsAdamW, optim.EftsRAdam)
    for cls in (optim.EftsAdam, optim.EftsAdamW, optim.EftsRAdam):
        assert issubclass(cls, optim.FlatOptimizer) and callable(cls.launch) and callable(cls.hyper_words)
    # bin/train.py constructs optimizers.<optimizer_type>(model, grad_norm=..., **optimizer_params): the reference's keyword names
    import inspect
    for cls, keys in ((optim.EftsAdam, {"lr", "betas", "eps", "weight_decay", "amsgrad"}), (optim.EftsAdamW, {"lr", "betas", "eps", "weight_decay", "amsgrad"}),
                      (optim.EftsRAdam, {"lr", "betas", "eps", "weight_decay"})):
        sig = inspect.signature(cls.__init__).parameters
        assert set(sig) == {"self", "model", "grad_norm"} | keys
    sig = inspect.signature(optim.EftsRAdam.__init__).parameters
    assert (sig["lr"].default, sig["betas"].default, sig["eps"].default, sig["weight_decay"].default) == (1e-3, (0.9, 0.999), 1e-8, 0)
    assert inspect.signature(optim.EftsAdamW.__init__).parameters["weight_decay"].default == 1e-2


def test_new_symbols_and_struct_pass_the_abi_checks(lib):
    """tests/test_abi_cpu.py's own checks, unchanged, see the new exports; the argument block's layout as gcc compiles the header"""
    import subprocess
    import tempfile
    from efficient_tts_amd import lib as L
    spec = importlib.util.spec_from_file_location("abi_checks", os.path.join(ROOT, "tests", "test_abi_cpu.py"))
    abi = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(abi)
    abi.test_header_symbols_are_exported(lib)
    abi.test_version_and_argument_errors(lib)
    abi.test_args_layouts_match_header()
    assert {"efts_optim_step", "efts_optim_hyper"} <= set(L.exported_symbols()) and L.ABI_VERSION == 602
    fields = [f for f, _ in L.OptimArgs._fields_]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "efts_abi.h"\nint main(){printf("%zu", sizeof(efts_optim_args));'
           + "".join(f'printf(" %zu", offsetof(efts_optim_args, {f}));' for f in fields)
           + 'printf(" %d %d %d", EFTS_OPTIM_ADAM, EFTS_OPTIM_ADAMW, EFTS_OPTIM_RADAM);return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        got = [int(v) for v in subprocess.check_output([os.path.join(d, "s")]).split()]
    assert got == [C.sizeof(L.OptimArgs)] + [getattr(L.OptimArgs, f).offset for f in fields] + [L.OPTIM_ADAM, L.OPTIM_ADAMW, L.OPTIM_RADAM]


def _f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


@pytest.mark.parametrize("step", [1, 5, 6, 1000])
def test_optim_hyper_equals_a_python_computation(lib, step):
    """efts_optim_hyper (host only): the four words, bit for bit the Python-float computation rounded to fp32 once"""
    lr, (b1, b2), _, wd = RECIPE
    arr = (C.c_float * 4)()
    for algo in (R.ADAM, R.ADAMW):
        assert lib.efts_optim_hyper(algo, lr, b1, b2, wd, step, arr) == 0
        want = [_f32(lr / (1.0 - b1 ** step)), _f32(math.sqrt(1.0 - b2 ** step)), 1.0 if algo == R.ADAM else _f32(1.0 - lr * wd), 0.0]
        assert list(arr) == want
    # AdamW's decay factor at a weight decay fp32 can see
    assert lib.efts_optim_hyper(R.ADAMW, lr, b1, b2, 1e-2, step, arr) == 0 and arr[2] == _f32(1.0 - lr * 1e-2) != 1.0
    # RADAM: N_sma, the branch and the step size as the reference computes them, in Python floats
    for beta2 in (0.99, 0.999):
        assert lib.efts_optim_hyper(R.RADAM, lr, b1, beta2, wd, step, arr) == 0
        _, rect, s = R.radam_rectification(step, beta2)
        assert list(arr) == [_f32(s / (1.0 - b1 ** step) * lr), 1.0, _f32(1.0 - wd * lr), 1.0 if rect else 0.0] and rect == (step >= 6)
    # ... and RADAM's decoupled decay at a weight decay fp32 can see (at the recipe's 1e-5, 1 - wd * lr rounds to 1.0f)
    assert lib.efts_optim_hyper(R.RADAM, lr, b1, b2, 1e-2, step, arr) == 0 and arr[2] == _f32(1.0 - 1e-2 * lr) != 1.0
    assert lib.efts_optim_hyper(R.RADAM, lr, b1, b2, 0.0, step, arr) == 0 and arr[2] == 1.0


def test_argument_errors_come_before_any_launch(lib):
    from efficient_tts_amd import lib as L
    arr = (C.c_float * 4)()
    assert lib.efts_optim_hyper(R.ADAM, 1e-3, 0.9, 0.99, 0.0, 0, arr) == -1                 # step < 1
    assert lib.efts_optim_hyper(3, 1e-3, 0.9, 0.99, 0.0, 1, arr) == -1                      # unknown algo
    assert lib.efts_optim_hyper(R.ADAM, 1e-3, 0.9, 0.99, 0.0, 1, None) == -1
    assert lib.efts_optim_step(None, None) == -1

    def args(**kw):
        a = L.OptimArgs()
        a.p, a.g, a.m, a.v, a.vmax, a.n, a.algo, a.amsgrad, a.beta1, a.beta2, a.step = 4096, 8192, 12288, 16384, 20480, 8, R.ADAM, 0, 0.9, 0.99, 1
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    for bad in (dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(n=0), dict(step=0), dict(algo=3), dict(algo=-1),
                dict(algo=R.RADAM, amsgrad=1), dict(amsgrad=1, vmax=None), dict(beta2=1.0)):
        assert lib.efts_optim_step(args(**bad), None) == -1, bad
    assert b"amsgrad" in lib.efts_last_error() or b"beta" in lib.efts_last_error()
    for bad in (dict(p=4100), dict(g=8196), dict(m=12292), dict(v=16388), dict(amsgrad=1, vmax=20484)):
        assert lib.efts_optim_step(args(**bad), None) == -3, bad
    with pytest.raises(ValueError):
        L.check(lib.efts_optim_step(args(n=-5), None), "efts_optim_step")


def test_constructors_refuse_an_fp32_model():
    from efficient_tts_amd import EfficientTTSCNN, optimizers
    model = EfficientTTSCNN(num_symbols=76, n_text_encoder_layer=1, n_mel_encoder_layer=1, n_decoder_layer=1, dropout_rate=0.0, use_masking=True,
                            precision="fp32")
    for cls, kw in ((optimizers.Adam, dict(amsgrad=False)), (optimizers.AdamW, {}), (optimizers.RAdam, {})):
        with pytest.raises(NotImplementedError, match="bf16x3"):
            cls(model, **kw)
