"""GPU (-m gpu): efts_optim_step -- clip + Adam / AdamW / RAdam in one launch over flat fp32 buffers -- against the float64 restatement of
tests/optim_reference.py, and the optimizers built on it (efficient_tts_amd/optim.py) through state dicts, the training loop, the
whole-step hipGraph and the command line.

Bounds of the kernel tests.  Nothing is fixed in advance: the unit is what fp32 arithmetic costs torch's OWN optimizer on the CPU on the
same inputs (optim_reference.fp32_gap: torch fp32 against the float64 restatement, as max |err| / max |ref| per tensor), for RAdam the
distance of the reference's recorded fp32 run from the restatement at the same hyper-parameters (tests/golden/radam_small.npz; torch
has no optimizer with that rule).  Only below the fixture's 1031 elements, where a maximum over a handful of elements underestimates
the worst case of a rounding error (at n = 1 it can be 0), is the unit the larger of that and the same measurement on the fixture's
inputs; from 1031 elements on it is the case's own inputs alone.  The device may use 4 units: its fused multiply-adds and its division
differ from the CPU's.  The measured device error is recorded beside DEVICE_UNITS below.

With the clip on, the unit of the moments grows with n (7e-6 at 524547 elements, 1.6e-4 at 4194563): torch's fp32 norm loses that much
summing millions of squares, and the clip coefficient scales every gradient.  The coefficient is one scalar per launch and has nothing to
do with where an element lies, so at the large sizes the clip-off cases (units near 2e-7) are the ones that hold the grid-stride loop."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import optim_reference as R

pytestmark = pytest.mark.gpu

DEVICE_UNITS = 4.0          # measured on an MI355X, worst over all cases: parameters 2.08, exp_avg 1.73, exp_avg_sq 1.80, max_exp_avg_sq 1.22 units
RECIPE = (1e-3, (0.9, 0.99), 1e-9, 1e-5)
ADAMW_DEFAULT = (1e-3, (0.9, 0.999), 1e-8, 1e-2)
RADAM_DEFAULT = (1e-3, (0.9, 0.999), 1e-8, 0.0)
RADAM_DECAY = (1e-3, (0.9, 0.99), 1e-9, 1e-2)       # the one RAdam setting whose decay factor 1 - lr * wd is not 1.0f (8 steps shrink p by 8e-5)
# (algo, amsgrad, hyper-parameters, RAdam fixture setting)
COMBOS = {"adam": (R.ADAM, False, RECIPE, None), "adam_ams": (R.ADAM, True, RECIPE, None), "adamw": (R.ADAMW, False, ADAMW_DEFAULT, None),
          "adamw_ams": (R.ADAMW, True, ADAMW_DEFAULT, None), "radam": (R.RADAM, False, RECIPE, "recipe"),
          "radam_default": (R.RADAM, False, RADAM_DEFAULT, "default"), "radam_decay": (R.RADAM, False, RADAM_DECAY, "decay")}
# a tail only; no multiple of 4; several blocks + tail; 513 blocks + tail; and, as one grid stride is 2048 blocks * 256 threads * 4 elements
# = 2097152, two full strides + a third, partial one + tail: the only size at which a thread runs the loop body more than once
SIZES = [1, 255, 4099, 524288 + 259, 2 * 2097152 + 259]
FIXTURE_N = 1031
STEPS = 8


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _inputs(n):
    """seeded N(0, 1) parameters and STEPS gradients (nowhere near eps in magnitude, where m / sqrt(v) is ill-conditioned)"""
    gen = torch.Generator().manual_seed(977 + n)
    p0, g = torch.randn(n, generator=gen).numpy(), torch.randn(STEPS, n, generator=gen).numpy()
    p0.setflags(write=False); g.setflags(write=False)
    return p0, g


def _reference(n, combo, max_norm):
    """(float64 restatement, unit) of one case"""
    algo, ams, hyper, setting = COMBOS[combo]
    p0, grads = _inputs(n)
    ref = R.run(algo, p0, grads, *hyper, amsgrad=ams, max_norm=max_norm)
    fx = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "radam_small.npz"))
    if algo == R.RADAM:
        h = fx[f"{setting}:hyper"]
        assert (float(h[0]), (float(h[1]), float(h[2])), float(h[3]), float(h[4])) == hyper
        tr, m, v, _ = R.run(R.RADAM, fx["p0"], fx["grads"], *hyper)
        unit = [R.relerr(fx[f"{setting}:params"], tr), R.relerr(fx[f"{setting}:exp_avg"], m), R.relerr(fx[f"{setting}:exp_avg_sq"], v)]
    else:
        unit = R.fp32_gap(algo, p0, grads, hyper, ams, max_norm, ref=ref)
        if n < FIXTURE_N:
            unit = [max(a, b) for a, b in zip(unit, R.fp32_gap(algo, fx["p0"], fx["grads"], hyper, ams, max_norm))]
    return ref, unit


def _device_run(combo, n, max_norm, words=False, steps=STEPS, sentinel=None):
    """STEPS launches of efts_optim_step from zero moments; returns (per-step parameters, m, v, vmax) as CPU tensors"""
    from efficient_tts_amd import lib as L, ops as P
    algo, ams, (lr, (b1, b2), eps, wd), _ = COMBOS[combo]
    lib, dev = L.load(), _dev()
    p0, grads = _inputs(n)
    p = torch.from_numpy(p0.copy()).to(dev)
    g = [torch.from_numpy(grads[t].copy()).to(dev) for t in range(steps)]        # (one allocation each: rows of a [steps][n] tensor are not 16-byte aligned)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    vmax = torch.zeros_like(p) if sentinel is None else torch.full_like(p, sentinel)
    sumsq = torch.zeros(1, device=dev)
    ws = torch.zeros(lib.efts_sumsq_workspace_bytes() // 4, device=dev)
    hw = torch.zeros(8, dtype=torch.int32, device=dev)
    traj = []
    with P.stream_scope():
        for t in range(1, steps + 1):
            a = L.OptimArgs()
            a.p, a.g, a.m, a.v, a.n = p.data_ptr(), g[t - 1].data_ptr(), m.data_ptr(), v.data_ptr(), n
            a.vmax = vmax.data_ptr() if (ams or sentinel is not None) else None
            a.max_norm, a.gscale, a.algo, a.amsgrad = max_norm, 1.0, algo, int(ams)
            a.lr, a.beta1, a.beta2, a.eps, a.weight_decay, a.step = lr, b1, b2, eps, wd, t
            if max_norm > 0:
                sumsq.zero_()
                L.check(lib.efts_sumsq(g[t - 1].data_ptr(), n, sumsq.data_ptr(), ws.data_ptr(), P._stream()), "efts_sumsq")
                a.sumsq = sumsq.data_ptr()
            if words:
                arr = (C.c_float * 4)()
                L.check(lib.efts_optim_hyper(algo, lr, b1, b2, wd, t, arr), "efts_optim_hyper")
                P.store_words(hw, [0, 0, 0, 0] + list((C.c_uint32 * 4).from_buffer(arr)))
                a.hyper, a.lr, a.step = hw.data_ptr() + 16, 0.0, 0
            L.check(lib.efts_optim_step(a, P._stream()), "efts_optim_step")
            traj.append(p.clone())
        torch.cuda.synchronize()
    return torch.stack(traj).cpu(), m.cpu(), v.cpu(), vmax.cpu()


@pytest.mark.parametrize("max_norm", [0.0, 1.0])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("combo", list(COMBOS))
def test_kernel_against_float64(combo, n, max_norm):
    """parameters of every step and the final moments of 8 steps, every algorithm / amsgrad combination, clip on and off"""
    ams = COMBOS[combo][1]
    ref, unit = _reference(n, combo, max_norm)
    got = _device_run(combo, n, max_norm)
    names = ["parameters", "exp_avg", "exp_avg_sq"] + (["max_exp_avg_sq"] if ams else [])
    err = [R.relerr(a.numpy(), b) for a, b in zip(got, ref) if b is not None]
    print(combo, n, max_norm, {k: f"{e:.3e} = {e / u:.2f} units" for k, e, u in zip(names, err, unit)})
    assert len(err) == len(unit) == len(names)
    for k, e, u in zip(names, err, unit):
        assert e <= DEVICE_UNITS * u, (k, e, u)
    if COMBOS[combo][0] == R.RADAM:
        # both branches ran: steps 1-5 plain, 6-8 rectified, by the words the launches were given
        from efficient_tts_amd import lib as L
        lr, (b1, b2), _, wd = COMBOS[combo][2]
        arr, flags = (C.c_float * 4)(), []
        for t in range(1, STEPS + 1):
            L.check(L.load().efts_optim_hyper(R.RADAM, lr, b1, b2, wd, t, arr), "efts_optim_hyper")
            flags.append(arr[3])
        assert flags == [0.0] * 5 + [1.0] * 3
        if max_norm == 0:
            # ... and it shows: with unit-size gradients the plain step 5 moves an element by 2.44 lr |m|, the rectified step 6 by
            # 0.042 lr |m| / sqrt(v), some thirty times less.  (Under the clip |m| shrinks with 1 / sqrt(n) while |m| / sqrt(v) does not, so
            # the two lengths say nothing there; the per-step parameters above are compared with the reference in either case.)
            tr = got[0].double()
            assert float((tr[5] - tr[4]).abs().max()) < 0.2 * float((tr[4] - tr[3]).abs().max())


@pytest.mark.parametrize("combo", list(COMBOS))
def test_device_words_equal_by_value_and_two_runs_equal(combo):
    """the four words of efts_optim_hyper in device memory against the by-value launch, steps 1..8, bit for bit; and no atomics:
    a second run gives the same bits"""
    for n in (4099, SIZES[-2], SIZES[-1]):
        a = _device_run(combo, n, 1.0)
        b = _device_run(combo, n, 1.0, words=True)
        c = _device_run(combo, n, 1.0)
        for x, y, z in zip(a[:3], b[:3], c[:3]):
            assert torch.equal(x, y) and torch.equal(x, z)
        if COMBOS[combo][1]:
            assert torch.equal(a[3], b[3]) and torch.equal(a[3], c[3])


@pytest.mark.parametrize("combo", ["adam", "adamw", "radam"])
def test_vmax_is_untouched_without_amsgrad(combo):
    for n in (255, SIZES[-2], SIZES[-1]):
        plain = _device_run(combo, n, 1.0, steps=2)
        with_buf = _device_run(combo, n, 1.0, steps=2, sentinel=-7.5)
        assert bool((with_buf[3] == -7.5).all())
        assert all(torch.equal(x, y) for x, y in zip(plain[:3], with_buf[:3]))


# ---------------------------------------------------------------------------------------------
# the optimizers on the model
# ---------------------------------------------------------------------------------------------
def _model(precision="bf16x3"):
    from efficient_tts_amd import EfficientTTSCNN
    from oracle import efts_oracle as O
    m = EfficientTTSCNN(num_symbols=76, dropout_rate=0.0, use_masking=True, sigma=0.01, precision=precision)
    m.load_state_dict(O.fill_params())
    return m.to(_dev()).eval()


def _tiny_batch(golden_dir):
    t = np.load(os.path.join(golden_dir, "fwd_tiny.npz"))
    return [torch.from_numpy(t[k]).to(_dev()) for k in ("text", "text_lengths", "speech", "speech_lengths")]


def _backward(model, opt, batch):
    text, tl, mel, sl = batch
    loss, stats, *_ = model(text=text, text_lengths=tl, speech=mel, speech_lengths=sl)
    opt.zero_grad()
    loss.backward()
    return stats


def test_amsgrad_adam_still_runs_its_own_kernel(golden_dir):
    """EftsAdam(amsgrad=True), the shipped recipe, for 3 steps against direct efts_sumsq + efts_adam_amsgrad calls on copies of the same
    buffers: bit for bit what it was before the family got a shared base"""
    from efficient_tts_amd import lib as L, ops as P
    from efficient_tts_amd.optim import EftsAdam, WarmupLR
    batch = _tiny_batch(golden_dir)
    m = _model()
    opt = EftsAdam(m, lr=1e-3, betas=(0.9, 0.99), eps=1e-9, weight_decay=1e-5, amsgrad=True, grad_norm=1.0)
    sch = WarmupLR(opt, warmup_steps=4000)
    lib, eng = L.load(), opt.eng
    for step in range(1, 4):
        _backward(m, opt, batch)
        p, m1, v, vm = opt.flat_p.clone(), opt.m.clone(), opt.v.clone(), opt.vmax.clone()
        lr = float(opt.param_groups[0]["lr"])
        opt.step()
        ss, ws = torch.zeros(1, device=_dev()), torch.zeros(lib.efts_sumsq_workspace_bytes() // 4, device=_dev())
        with P.stream_scope():
            L.check(lib.efts_sumsq(eng.flat.data_ptr(), eng.numel, ss.data_ptr(), ws.data_ptr(), P._stream()), "efts_sumsq")
            L.check(lib.efts_adam_amsgrad(p.data_ptr(), eng.flat.data_ptr(), m1.data_ptr(), v.data_ptr(), vm.data_ptr(), eng.numel, ss.data_ptr(),
                                          1.0, 1.0, lr, 0.9, 0.99, 1e-9, 1e-5, step, P._stream()), "efts_adam_amsgrad")
            torch.cuda.synchronize()
        assert opt.t == step and torch.equal(p, opt.flat_p) and torch.equal(m1, opt.m) and torch.equal(v, opt.v) and torch.equal(vm, opt.vmax)
        assert not torch.equal(vm, torch.zeros_like(vm))
        sch.step()
    sd = opt.state_dict()
    assert list(sd["state"][0]) == ["step", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"] and sd["param_groups"][0]["amsgrad"] is True
    assert len(opt.hyper_words(4)) == 3 and opt.hyper_word0 == 0


class _ReferenceLayout(torch.optim.Optimizer):
    """an optimizer with the reference RAdam's defaults and torch.optim.Optimizer's own state_dict / load_state_dict, which that class inherits"""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))


@pytest.mark.parametrize("kind", ["adam", "adamw", "radam"])
def test_state_dict_round_trips(golden_dir, kind):
    """state_dict() has the layout of the optimizer each class replaces, numbered in model.parameters() order: the stock optimizer loads
    ours, ours loads the stock one's, and a resumed optimizer fed the same gradients continues with the same bits"""
    from efficient_tts_amd import optim as OP
    kw = dict(lr=1e-3, betas=(0.9, 0.99), eps=1e-9, weight_decay=1e-5)
    make, stock = {"adam": (lambda mm: OP.EftsAdam(mm, amsgrad=False, grad_norm=1.0, **kw), lambda ps: torch.optim.Adam(ps, amsgrad=False, **kw)),
                   "adamw": (lambda mm: OP.EftsAdamW(mm, grad_norm=1.0, **kw), lambda ps: torch.optim.AdamW(ps, **kw)),
                   "radam": (lambda mm: OP.EftsRAdam(mm, grad_norm=1.0, **kw), lambda ps: _ReferenceLayout(ps, **kw))}[kind]
    batch = _tiny_batch(golden_dir)
    m = _model()
    opt = make(m)
    assert opt.vmax is None
    for _ in range(2):
        _backward(m, opt, batch)
        opt.step()
    sd = opt.state_dict()
    params = list(m.parameters())
    assert set(sd["state"].keys()) == set(range(len(params))) and sd["param_groups"][0]["params"] == list(range(len(params)))
    for i, p in enumerate(params):
        st = sd["state"][i]
        assert set(st) == {"step", "exp_avg", "exp_avg_sq"} and st["exp_avg"].shape == p.shape and st["exp_avg_sq"].shape == p.shape
        if kind == "radam":
            assert type(st["step"]) is int and st["step"] == 2
        else:
            assert torch.is_tensor(st["step"]) and float(st["step"]) == 2.0
    assert {"lr", "betas", "eps", "weight_decay", "params"} <= set(sd["param_groups"][0])
    if kind == "radam":
        assert set(sd["param_groups"][0]) == {"lr", "betas", "eps", "weight_decay", "params"}
    else:
        assert sd["param_groups"][0]["amsgrad"] is False
    ref = stock(params)
    ref.load_state_dict(sd)
    rs = ref.state_dict()
    assert torch.equal(rs["state"][3]["exp_avg_sq"], sd["state"][3]["exp_avg_sq"]) and torch.equal(rs["state"][0]["exp_avg"], sd["state"][0]["exp_avg"])
    # a second model + optimizer resumed from the stock optimizer's dict continues bit-identically on the same gradients
    m2 = _model()
    m2.load_state_dict(m.state_dict())
    opt2 = make(m2)
    opt2.load_state_dict(rs)
    assert opt2.t == opt.t == 2 and torch.equal(opt2.m, opt.m) and torch.equal(opt2.v, opt.v)
    for (n, a), (_, b) in zip(m.named_parameters(), m2.named_parameters()):      # (not flat_p as a whole: its padding to a multiple of 4 elements is never written)
        assert torch.equal(a, b), ("before the step", n)
    _backward(m, opt, batch)
    _backward(m2, opt2, batch)
    opt2.eng.flat.copy_(opt.eng.flat)          # (two backward passes differ in the last bits: float atomics in the weight gradients)
    opt.step(); opt2.step()
    torch.cuda.synchronize()
    assert opt2.t == 3 and torch.equal(opt2.m, opt.m) and torch.equal(opt2.v, opt.v)
    for (n, a), (_, b) in zip(m.named_parameters(), m2.named_parameters()):
        assert torch.equal(a, b), n
    assert not torch.equal(opt.m, torch.zeros_like(opt.m))


def test_three_training_steps_adamw_against_stock_torch(golden_dir):
    """trainer.py:139-160 x3 (fwd, bwd, clip 1.0, AdamW, WarmupLR 4000): EftsAdamW against stock torch.optim.AdamW + clip_grad_norm_ on the
    gradients our backward hands to autograd -- the two arms and the tolerances of test_gpu_train.test_three_training_steps_match_reference"""
    from efficient_tts_amd.optim import EftsAdamW, WarmupLR
    batch = _tiny_batch(golden_dir)
    kw = dict(lr=1e-3, betas=(0.9, 0.99), eps=1e-9, weight_decay=1e-2)
    out = {}
    for fused in (False, True):
        m = _model()
        opt = EftsAdamW(m, grad_norm=1.0, **kw) if fused else torch.optim.AdamW(m.parameters(), **kw)
        sch = WarmupLR(opt, warmup_steps=4000)
        losses = []
        for step in range(3):
            stats = _backward(m, opt, batch)
            if not fused:
                torch.nn.utils.clip_grad_norm_(m.parameters(), 1.0)
            opt.step()
            sch.step()
            losses.append(stats["loss"])
        out[fused] = (losses, {n: p.detach().cpu().numpy().copy() for n, p in m.named_parameters()})
    for a, b in zip(out[True][0], out[False][0]):
        assert abs(a - b) <= 1e-3 * b, out
    init = {n: p.detach().cpu().numpy() for n, p in _model().named_parameters()}
    moved = 0.0
    for n, ref in out[False][1].items():
        assert np.abs(out[True][1][n] - ref).max() <= 2e-6 + 1e-4 * np.abs(ref).max(), n
        moved = max(moved, float(np.abs(ref - init[n]).max()))
    assert moved > 1e-6                          # (the parameters did move: three steps at the warm-up's learning rates)


def test_graphed_radam_step_equals_the_eager_loop():
    """step_graph.GraphedStep with EftsRAdam for 8 steps -- the replayed words cross the rectification switch at step 6 -- against the eager
    loop.  Bounds and reasoning of test_gpu_train.test_graphed_training_step_equals_the_eager_loop: the backward's float atomics make two
    runs differ by ~2e-8 in the gradients, so the 8-step comparison is loose (losses to 3e-3, moments to 5e-2 in norm, parameters within
    half a learning rate, host counters exactly) and the tight part is ONE step from one and the same state, here step 6, the first
    rectified one: a replay that still held step 5's words would move almost every parameter by the difference of the two rules."""
    from efficient_tts_amd import EfficientTTSCNN
    from efficient_tts_amd.optim import EftsRAdam, WarmupLR
    from efficient_tts_amd.step_graph import GraphedStep
    dev = _dev()
    B, T1, T2 = 3, 40, 130
    gen = torch.Generator().manual_seed(B * 31 + T2)
    batches = []
    for _ in range(2):
        batches.append((torch.randint(0, 76, (B, T1), generator=gen).to(dev), torch.randint(T1 // 2, T1 + 1, (B,), generator=gen).to(dev),
                        torch.randn(B, T2, 80, generator=gen).to(dev), torch.randint(T2 // 2, T2 + 1, (B,), generator=gen).to(dev)))

    def fresh(lr):
        torch.manual_seed(1)
        m = EfficientTTSCNN(num_symbols=76, dropout_rate=0.0, use_masking=True, sigma=0.01, precision="bf16").to(dev).train()
        return m, EftsRAdam(m, lr=lr, betas=(0.9, 0.99), eps=1e-9, weight_decay=1e-5, grad_norm=1.0)

    def run(graphed):
        m, opt = fresh(1e-3)
        sch = WarmupLR(opt, warmup_steps=50)
        step = GraphedStep(m, opt, sch)
        losses = []
        for i in range(8):
            a = batches[i % 2]
            loss, _ = step(*a) if graphed else step._eager(*a)
            losses.append(float(loss))
        assert step.replays == (7 if graphed else 0)                 # the capture really happened (the first call runs eagerly)
        return losses, {n: p.detach().clone() for n, p in m.named_parameters()}, (opt.m.clone(), opt.v.clone(), opt.t), sch.last_epoch

    la, pa, sa, ea = run(False)
    lb, pb, sb, eb = run(True)
    assert ea == eb and sa[2] == sb[2] == 8
    for x, y in zip(la, lb):
        assert abs(x - y) <= 3e-3 * abs(x), (la, lb)
    for x, y in zip(sa[:2], sb[:2]):
        assert float((x - y).double().norm()) <= 5e-2 * float(x.double().norm())
    for n in pa:
        assert float((pa[n] - pb[n]).abs().max()) <= 0.5 * 1e-3, n
    # the tight part: steps 5 (plain) and 6 (rectified) from one and the same state, eager against replayed
    lr = 1e-4
    m, opt = fresh(lr)
    step = GraphedStep(m, opt, None)
    a = batches[0]
    for _ in range(4):
        step(*a)
    assert opt.t == 4 and step.replays == 3
    eng = opt.eng
    for t in (5, 6):
        state = (opt.flat_p.clone(), opt.m.clone(), opt.v.clone(), opt.t, m.dropout_calls)
        le, _ = step._eager(*a)
        ge, pe = eng.flat.clone(), opt.flat_p.clone()
        opt.flat_p.copy_(state[0]); opt.m.copy_(state[1]); opt.v.copy_(state[2])
        opt.t, m.dropout_calls = state[3], state[4]
        m.planes.invalidate()
        n0 = step.replays
        lg, _ = step(*a)
        assert step.replays == n0 + 1 and opt.t == t
        gg, pg = eng.flat.clone(), opt.flat_p.clone()
        assert float(le) == float(lg)
        assert float((ge - gg).double().norm()) <= 1e-6 * float(ge.double().norm())
        d = (pe - pg).abs()
        moved = (pe - state[0]).abs()
        # how far one step can move an element.  Step 5 (plain): |m / (1 - beta1^5)| <= the largest gradient element <= the clipped norm 1,
        # so lr.  Step 6 (rectified): |m| / sqrt(v) <= 1 / sqrt(1 - beta2) = 10, times lr * step size (0.0422 at step 6).  Both plus the
        # decay lr * wd * |p| and 1 % for fp32.
        reach = (10 * 0.0423 * lr if t == 6 else lr) * 1.01 + 1e-5 * lr * float(state[0].abs().max())
        assert float(moved.max()) <= reach
        assert float(d.max()) <= 2 * reach and float((d <= 1e-7).float().mean()) >= 0.999
        if t == 6:      # (the check can tell the rules apart: step 5's rule at step 6 would have moved most elements somewhere else)
            plain = lr / (1 - 0.9 ** 6) * opt.m.abs()
            assert float(((moved - plain).abs() > 1e-7).float().mean()) > 0.5


@pytest.mark.parametrize("optimizer,graph", [("RAdam", True), ("AdamW", False)])
def test_cli_trains_and_resumes_with_the_new_optimizers(tmp_path, optimizer, graph):
    """python -m efficient_tts_amd.bin.train with `optimizer_type: RAdam` / `AdamW` in the reference's YAML schema (in the manner of
    tests/test_cli_data.py): trains, saves the optimizer's own state layout, resumes from its own checkpoint"""
    import yaml
    from efficient_tts_amd.bin.train import main
    params = dict(RAdam=dict(lr=1.0e-3, betas=[0.9, 0.99], eps=1.0e-9, weight_decay=1.0e-5),
                  AdamW=dict(lr=1.0e-3, betas=[0.9, 0.99], eps=1.0e-9, weight_decay=1.0e-2, amsgrad=False))[optimizer]
    cfg = dict(dataset_type="SyntheticTextAudio", dataset_params=dict(n_items=12, min_phones=8, max_phones=16),
               collate_fn_type="TextMelCollate", model_name="EfficientTTSCNN",
               model_params=dict(num_symbols=76, dropout_rate=0.0, use_masking=True, use_weighted_masking=False, sigma=0.01),
               batch_size=4, pin_memory=False, num_workers=0, optimizer_type=optimizer, optimizer_params=params, grad_norm=1.0,
               scheduler_type="WarmupLR", scheduler_params=dict(warmup_steps=4000), train_max_steps=6, save_interval_steps=3,
               eval_interval_steps=3, log_interval_steps=2, bucket_frames=32, bucket_phones=8, graph_steps=graph)
    path, out, out2 = tmp_path / "c.yaml", tmp_path / "exp", tmp_path / "exp2"
    with open(path, "w") as f:
        yaml.dump(cfg, f)
    assert main(["--outdir", str(out), "--config", str(path), "--verbose", "0"]) == 0
    ck3, ck6 = out / "checkpoint-3steps.pkl", out / "checkpoint-6steps.pkl"
    assert ck3.exists() and ck6.exists()
    sd3, sd6 = torch.load(ck3, map_location="cpu"), torch.load(ck6, map_location="cpu")
    assert set(sd6) == {"model", "optimizer", "scheduler", "steps", "epochs"} and sd6["steps"] == 6
    st = sd6["optimizer"]["state"][0]
    assert set(st) == {"step", "exp_avg", "exp_avg_sq"} and int(float(st["step"])) == 6 and (type(st["step"]) is int) == (optimizer == "RAdam")
    assert all(torch.isfinite(v).all() for v in sd6["model"].values())
    assert any(not torch.equal(sd3["model"][k], sd6["model"][k]) for k in sd6["model"])
    assert main(["--outdir", str(out2), "--config", str(path), "--verbose", "0", "--resume", str(ck3)]) == 0
    sd2 = torch.load(out2 / "checkpoint-6steps.pkl", map_location="cpu")
    assert sd2["steps"] == 6 and not (out2 / "checkpoint-3steps.pkl").exists()
    assert int(float(sd2["optimizer"]["state"][0]["step"])) == 6
