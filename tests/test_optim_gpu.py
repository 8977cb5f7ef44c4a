"""The optimiser step on the MI355X: vfi_amd.optim's SGD, Adam, Adamax and RMSprop against torch.optim
in float64 on the CPU from the same float32 inputs, at the sizes where csrc/vfi_optim.hip takes another path.

Sizes come from the limits entry (C elements per chunk, T tensors and K chunks per launch): single tensors of 1, 3, 4, 5,
C - 1, C, C + 1 and 2C + 3 elements, a parameter that is a view one element into its storage (4-byte aligned: the scalar
path), the same with only the grad misaligned, T + 1 tensors (two launches), and a set of more than K chunks in which a
tensor continues in the second launch.

Bound, per tensor (parameter or state) and step: with e32 the max abs error of torch.optim's own float32 CPU step against
the float64 run, the kernel's max abs error is at most 2 e32 + one ulp of max |p|; for a state tensor the ulp is that of
max |state| where that is the smaller one, so the bound is never wider than "one ulp of max |p|".  Every case prints its
largest err / allowance before it asserts."""
import copy

import numpy as np
import pytest
import torch

import adversarial_ref as AR
from oracle import nets_cpu
from vfi_amd import ops, optim
from vfi_amd.adacof.losses import adversarial
from vfi_amd.fusion_net.fusion_net import FusionNet

pytestmark = pytest.mark.gpu

C, T, K, MAX_NUMEL = ops.optim_limits()
SINGLE = (1, 3, 4, 5, C - 1, C, C + 1, 2 * C + 3)
STATE_KEYS = ("momentum_buffer", "exp_avg", "exp_avg_sq", "exp_inf", "square_avg")

CONFIGS = {
    "sgd": (optim.SGD, dict(lr=0.1)),
    "sgd-wd": (optim.SGD, dict(lr=0.1, weight_decay=1e-2)),
    "sgd-momentum": (optim.SGD, dict(lr=0.1, momentum=0.9)),                       # utility.make_optimizer's SGD
    "sgd-momentum-wd": (optim.SGD, dict(lr=0.1, momentum=0.9, weight_decay=1e-2)),
    "sgd-nesterov": (optim.SGD, dict(lr=0.1, momentum=0.9, nesterov=True, weight_decay=1e-2)),
    "adam": (optim.Adam, dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8)),
    "adam-wd": (optim.Adam, dict(lr=1e-3, weight_decay=1e-2)),
    "adam-wgan-gp": (optim.Adam, dict(lr=1e-5, betas=(0.0, 0.9), eps=1e-8)),       # Adversarial's fixed Adam
    "adamax": (optim.Adamax, dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8)),
    "adamax-wd": (optim.Adamax, dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)),
    # beta2 = 0 is the one way u falls to eps under a non-zero m: u = max(0 u, |g| + eps) = eps at g = 0, m = beta1 m
    "adamax-beta2-0": (optim.Adamax, dict(lr=1e-3, betas=(0.9, 0.0), eps=1e-8)),
    "rmsprop": (optim.RMSprop, dict(lr=1e-3, eps=1e-8)),
    "rmsprop-wd": (optim.RMSprop, dict(lr=1e-3, eps=1e-8, weight_decay=1e-2)),
}
ONE_PER_KIND = ("sgd-nesterov", "adam-wd", "adamax-wd", "rmsprop-wd")


def _parent(cls):
    return getattr(torch.optim, cls.__name__)


def _inputs(seed, sizes, steps=3, zeros=True):
    """-> (start, grads): float32 CPU tensors; grads[step][i].  With `zeros`, element 0 of every grad is exactly 0 in the first
    two steps (m = 0 over Adamax's u = eps and Adam's denominator eps) and ordinary in the third; element n // 2 is exactly 0
    in the second step only, after an ordinary first one (m != 0; with beta2 = 0 Adamax then divides it by u = eps)."""
    g = torch.Generator().manual_seed(seed)
    start = [torch.randn(n, generator=g) * 1.5 for n in sizes]
    grads = []
    for s in range(steps):
        row = [torch.randn(n, generator=g) for n in sizes]
        if zeros and s < 2:
            for t in row:
                t[0] = 0.0
                if s == 1:
                    t[t.numel() // 2] = 0.0
        grads.append(row)
    return start, grads


def _place(t, device, dtype, misaligned=False):
    if device is None:
        return t.to(dtype).clone()
    if not misaligned:
        out = t.to(device).clone()
        assert out.data_ptr() % 16 == 0
        return out
    base = torch.empty(t.numel() + 1, device=device)
    out = base[1:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


def _snapshot(opt, params):
    ps = [p.detach().to("cpu", torch.float64, copy=True) for p in params]
    st = [{k: v.detach().to("cpu", torch.float64, copy=True) for k, v in opt.state.get(p, {}).items() if k in STATE_KEYS} for p in params]
    steps = [float(opt.state[p]["step"]) if "step" in opt.state.get(p, {}) else None for p in params]
    return ps, st, steps


def _run(cls, kw, start, grads, device=None, dtype=torch.float32, views=None, clamp=None, between=None, opt_hook=None):
    """The optimiser `cls(**kw)` over `start` for len(grads) steps; a None grad skips that parameter in that step.
    device None: on the CPU in `dtype`.  views: {index: "param" | "grad"} puts that tensor one element into its storage.
    between(opt, step) runs after each step (a scheduler).  -> [(params, states, step counts) after each step], opt, params."""
    views = views or {}
    params = [_place(t, device, dtype, views.get(i) == "param").requires_grad_(True) for i, t in enumerate(start)]
    opt = cls(params, **kw)
    if opt_hook is not None:
        opt_hook(opt)
    out = []
    for s, row in enumerate(grads):
        for i, (p, g) in enumerate(zip(params, row)):
            p.grad = None if g is None else _place(g, device, dtype, views.get(i) == "grad")
        if clamp is None:
            opt.step()
        else:
            opt.step(clamp=clamp)
        if between is not None:
            between(opt, s)
        out.append(_snapshot(opt, params))
    return out, opt, params


def _ulp(x):
    return float(np.spacing(np.float32(abs(x))))


def _within_bound(what, got, ref32, ref64):
    """got, ref32, ref64: the [(params, states, counts)] lists of _run.  -> the largest err / allowance, asserted <= 1."""
    worst = (0.0, None)
    for s, ((gp, gs, gc), (ap, as_, ac), (dp, ds, dc)) in enumerate(zip(got, ref32, ref64)):
        assert gc == dc == ac, (what, s, gc, dc)
        for i in range(len(dp)):
            ulp_p = _ulp(float(dp[i].abs().max()))
            rows = [("param", gp[i], ap[i], dp[i], ulp_p)]
            assert gs[i].keys() == ds[i].keys(), (what, s, i, gs[i].keys(), ds[i].keys())
            for k in ds[i]:
                rows.append((k, gs[i][k], as_[i][k], ds[i][k], min(ulp_p, _ulp(float(ds[i][k].abs().max())))))
            for name, g_, a_, d_, ulp in rows:
                assert g_.shape == d_.shape and bool(torch.isfinite(g_).all())
                err, e32 = float((g_ - d_).abs().max()), float((a_ - d_).abs().max())
                allow = 2.0 * e32 + ulp
                if err / allow > worst[0]:
                    worst = (err / allow, (s, i, name, err, e32, ulp))
    print(f"{what}: worst err / allowance {worst[0]:.3f} at (step, tensor, what, err, e32, ulp) = {worst[1]}")
    assert worst[0] <= 1.0, (what, worst)
    return worst[0]


def _three_ways(what, cls, kw, start, grads, device, views=None, **more):
    got, opt, params = _run(cls, kw, start, grads, device, views=views, **more)
    ref32, _, _ = _run(_parent(cls), kw, start, grads, None, torch.float32, **more)
    ref64, _, _ = _run(_parent(cls), kw, start, grads, None, torch.float64, **more)
    _within_bound(what, got, ref32, ref64)
    return got, opt, params


# ---- against float64 --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_single_tensor_sizes_and_views_against_float64(device, name):
    """Three consecutive steps (the first SGD-momentum step among them) of one optimiser over the eight sizes plus the two
    misaligned tensors, all in one multi-tensor call per step."""
    cls, kw = CONFIGS[name]
    sizes = SINGLE + (C + 7, C + 7)
    views = {len(SINGLE): "param", len(SINGLE) + 1: "grad"}
    start, grads = _inputs(11, sizes)
    _three_ways(name, cls, kw, start, grads, device, views)


@pytest.mark.parametrize("name", ONE_PER_KIND)
def test_more_tensors_than_a_launch_holds(device, name):
    cls, kw = CONFIGS[name]
    start, grads = _inputs(12, [1 + (7 * i) % 23 for i in range(T + 1)])
    _three_ways(f"{name}, {T + 1} tensors", cls, kw, start, grads, device)


@pytest.mark.parametrize("name", ONE_PER_KIND)
def test_more_chunks_than_a_launch_holds(device, name):
    """K - 1 chunks, then a tensor of four chunks of which the first is the launch's last and three go to the next launch
    (with a partial last chunk), then a small tensor."""
    cls, kw = CONFIGS[name]
    sizes = ((K - 2) * C + 7, 3 * C + 1, 5)
    assert sum(-(-n // C) for n in sizes) > K
    start, grads = _inputs(13, sizes, steps=2)
    _three_ways(f"{name}, {sum(-(-n // C) for n in sizes)} chunks", cls, kw, start, grads, device)


def test_element_offsets_beyond_2_to_31(device):
    """One tensor of 2^31 + C + 5 elements through plain SGD (two arrays of 8.6 GB): a 32-bit element offset would wrap.  Checked
    on the head, the elements around 2^31, the tail and every 65537th element.  p - lr g rounds the product and the sum once
    each: the error is below one ulp of max |p|."""
    n = 2 ** 31 + C + 5
    assert n <= MAX_NUMEL
    p = torch.rand(n, device=device).requires_grad_(True)
    g = torch.rand(n, device=device)
    pick = [slice(0, 16), slice(2 ** 31 - C - 3, 2 ** 31 + 5), slice(n - C - 5, n), slice(None, None, 65537)]
    before = [(p.detach()[s].cpu().double(), g[s].cpu().double()) for s in pick]
    p.grad = g
    opt = optim.SGD([p], lr=0.25)
    opt.step()
    torch.cuda.synchronize()
    for s, (p0, g0) in zip(pick, before):
        want = p0 - 0.25 * g0
        err = float((p.detach()[s].cpu().double() - want).abs().max())
        print(f"slice {s}: max abs err {err:.3e}")
        assert err <= _ulp(1.0), (s, err)
    assert torch.equal(g[pick[3]].cpu().double(), before[3][1])


# ---- which parameters advance -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("adam", "adamax", "rmsprop", "sgd-momentum"))
def test_skipped_parameter_keeps_its_own_step_count(device, name):
    cls, kw = CONFIGS[name]
    start, grads = _inputs(14, (C + 5, 37, 2 * C))
    grads[0][1] = None                                       # step 1 without tensor 1: steps 2 and 3 hold two distinct counts
    got, opt, params = _three_ways(name, cls, kw, start, grads, device)
    assert torch.equal(got[0][0][1].float(), start[1]) and got[0][1][1] == {}
    if cls is not optim.SGD:
        assert got[0][2] == [1.0, None, 1.0] and got[1][2] == [2.0, 1.0, 2.0] and got[2][2] == [3.0, 2.0, 3.0]


def test_scheduler_changes_the_next_update(device):
    cls, kw = CONFIGS["adamax"]
    start, grads = _inputs(15, (C + 1, 9))
    sched = {}

    def hook(opt):
        sched[id(opt)] = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.1)

    def between(opt, s):
        sched[id(opt)].step()

    got, opt, _ = _three_ways("adamax + StepLR", cls, kw, start, grads, device, opt_hook=hook, between=between)
    assert opt.param_groups[0]["lr"] == pytest.approx(1e-6)
    fixed, _, _ = _run(cls, kw, start, grads, device)
    assert not torch.equal(fixed[1][0][0], got[1][0][0])


def test_a_failed_first_sgd_step_leaves_no_momentum_buffer(device, monkeypatch):
    """The buffers of a first step are made before the launch; when the launch raises they must not stay behind as if they
    held a momentum: the next step is still the first (buf = g) and gives the float64 result."""
    cls, kw = CONFIGS["sgd-momentum"]
    start, grads = _inputs(19, (C + 3, 6), steps=1)
    params = [t.to(device).requires_grad_(True) for t in start]
    opt = cls(params, **kw)
    for p, g in zip(params, grads[0]):
        p.grad = g.to(device)

    def broken(*a, **k):
        raise RuntimeError("launch refused")
    with monkeypatch.context() as m:
        m.setattr(ops, "optim_step", broken)
        with pytest.raises(RuntimeError, match="launch refused"):
            opt.step()
    assert all("momentum_buffer" not in opt.state[p] for p in params)
    assert all(torch.equal(p.detach().cpu(), t) for p, t in zip(params, start))
    opt.step()
    ref32, _, _ = _run(_parent(cls), kw, start, grads, None, torch.float32)
    ref64, _, _ = _run(_parent(cls), kw, start, grads, None, torch.float64)
    _within_bound("sgd-momentum after a failed launch", [_snapshot(opt, params)], ref32, ref64)


# ---- clamp, repeatability ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ONE_PER_KIND + ("sgd",))
def test_clamp_in_the_pass_is_clamp_afterwards(device, name):
    cls, kw = CONFIGS[name]
    sizes = (5, C + 1, 2 * C + 3, C + 7)
    start, grads = _inputs(16, sizes, steps=1)
    fused, _, _ = _run(cls, kw, start, grads, device, views={3: "param"}, clamp=(-1, 1))
    plain, _, params = _run(cls, kw, start, grads, device, views={3: "param"})
    assert any(float(p.detach().abs().max()) > 1 for p in params)
    for i, p in enumerate(params):
        with torch.no_grad():
            p.clamp_(-1, 1)
        assert torch.equal(p.detach().cpu().double(), fused[0][0][i]), (name, i)
    assert all(torch.equal(a[k], b[k]) for a, b in zip(fused[0][1], plain[0][1]) for k in a)


@pytest.mark.parametrize("name", ONE_PER_KIND)
def test_a_step_repeats_its_bits(device, name):
    cls, kw = CONFIGS[name]
    start, grads = _inputs(17, (3 * C + 2, 7, C))
    a, _, _ = _run(cls, kw, start, grads, device, views={1: "param"})
    b, _, _ = _run(cls, kw, start, grads, device, views={1: "param"})
    for (ap, as_, _), (bp, bs, _) in zip(a, b):
        assert all(torch.equal(x, y) for x, y in zip(ap, bp))
        assert all(torch.equal(x[k], y[k]) for x, y in zip(as_, bs) for k in x)


# ---- state_dict interchange with the parent class --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("sgd-momentum-wd", "adam-wd", "adamax-wd", "rmsprop-wd"))
@pytest.mark.parametrize("direction", ("device-to-parent", "parent-to-device"))
def test_state_dict_interchanges_with_the_parent_class(device, name, direction):
    """Two steps with one class, its state_dict loaded into the other class over copies of the parameters, the third step
    there, in float32 on the GPU: within the bound of the float64 run of all three steps."""
    cls, kw = CONFIGS[name]
    first, second = (cls, _parent(cls)) if direction == "device-to-parent" else (_parent(cls), cls)
    start, grads = _inputs(18, (C + 3, 11, 2 * C))
    ref32, _, _ = _run(_parent(cls), kw, start, grads, None, torch.float32)
    ref64, _, _ = _run(_parent(cls), kw, start, grads, None, torch.float64)
    two, opt, params = _run(first, kw, start, grads[:2], device)
    copies = [p.detach().clone().requires_grad_(True) for p in params]
    other = second(copies, **kw)
    other.load_state_dict(copy.deepcopy(opt.state_dict()))      # (load_state_dict keeps tensors of the right dtype and device as they are)
    assert type(other) is second and type(other) is not type(opt)
    for p, g in zip(copies, grads[2]):
        p.grad = g.to(device)
    other.step()
    _within_bound(f"{name}, {direction}", [_snapshot(other, copies)], ref32[2:], ref64[2:])
    if first is cls:                                      # the device class's own third step from the same state
        for p, g in zip(params, grads[2]):
            p.grad = g.to(device)
        opt.step()
        _within_bound(f"{name}, third device step", [_snapshot(opt, params)], ref32[2:], ref64[2:])


# ---- version counters -------------------------------------------------------------------------------------------------------
def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def test_version_counters_move_and_the_packed_weights_follow(device):
    """FusionNet (batch 1, 16 x 16) keeps packed copies of its weights keyed on the parameters' version counters.  After a
    device step its forward is that of a twin loaded with the float64-stepped weights, to the relative L2 of 2e-4 that
    tests/test_fusionnet_backward_gpu.py holds the HIP passes to, and it is not the forward from before the step."""
    sd = nets_cpu.fusionnet_random_state_dict(8, uncertainty_maps=3)
    net = FusionNet(uncertainty_maps=3).to(device)
    net.load_state_dict(sd)
    net.train(True)
    g = torch.Generator().manual_seed(4)
    ins = [torch.rand((1, c, 16, 16), generator=g).to(device) for c in (3, 3, 3, 6, 3)]
    with torch.no_grad():
        before = net(*ins).clone()
    torch.nn.functional.l1_loss(net(*ins), ins[1]).backward()
    named = [(k, p) for k, p in net.named_parameters() if p.grad is not None]
    assert len(named) >= 7
    kw = dict(lr=1e-3)
    opt = optim.Adam([p for _, p in named], **kw)
    versions = [p._version for _, p in named]
    start = [p.detach().cpu().clone() for _, p in named]
    grads = [p.grad.cpu().clone() for _, p in named]
    opt.step()
    assert all(p._version > v for (_, p), v in zip(named, versions))
    with torch.no_grad():
        after = net(*ins).clone()
    p64 = [t.double().requires_grad_(True) for t in start]
    for p, gr in zip(p64, grads):
        p.grad = gr.double()
    torch.optim.Adam(p64, **kw).step()
    twin_sd = {k: v.clone() for k, v in net.state_dict().items()}
    for (k, _), p in zip(named, p64):
        assert not torch.equal(p.detach().float(), sd[k].float())
        twin_sd[k] = p.detach().float()
    twin = FusionNet(uncertainty_maps=3).to(device)
    twin.load_state_dict(twin_sd)
    twin.train(True)
    with torch.no_grad():
        want = twin(*ins)
    print(f"forward after the step vs the float64-stepped twin: {_rel(after, want):.3e}; vs before: {_rel(after, before):.3e}; "
          f"{float(((after > 0) & (after < 1)).float().mean()):.2f} of the output inside the clamp")
    assert _rel(after, want) <= 2e-4
    assert _rel(after, before) >= 2e-3            # ten times the tolerance: the twin is told from the stale forward


# ---- the AdaCoF trainer's discriminator update ------------------------------------------------------------------------------
def _adversarial_update(gan_type, flag, device):
    torch.manual_seed(31)
    adv = adversarial.Adversarial(AR.args(16, gradient_penalty=True, device_optimizer=flag), gan_type)
    with torch.no_grad():                       # beyond [-1, 1]: WGAN's clamp moves it
        adv.discriminator.classifier[2].bias.fill_(1.5)
    adv = adv.to(device)
    every = list(adv.discriminator.parameters())
    before = [p.detach().cpu().clone() for p in every]
    g = torch.Generator().manual_seed(32)
    fake, real = (torch.rand((2, 3, 16, 16), generator=g).to(device) for _ in range(2))
    torch.manual_seed(33)
    adv(fake, real)
    params = [p for p in every if p.grad is not None]
    assert len(params) >= 12
    start = [b for b, p in zip(before, every) if p.grad is not None]
    return adv, start, [p.grad.cpu().clone() for p in params], [p.detach().cpu().double() for p in params]


@pytest.mark.parametrize("gan_type", ("WGAN", "WGAN_GP"))
def test_adversarial_update_with_and_without_the_flag(device, gan_type):
    """One discriminator update from the same seed with torch's optimiser and with the device class.  Each run's parameters
    against the float64 step from that run's own start and gradients: the device run's error is within 2 x the torch run's
    plus one ulp of max |p|."""
    runs = {flag: _adversarial_update(gan_type, flag, device) for flag in (False, True)}
    assert type(runs[False][0].optimizer) is (torch.optim.Adam if gan_type == "WGAN_GP" else torch.optim.Adamax)
    assert type(runs[True][0].optimizer) is (optim.Adam if gan_type == "WGAN_GP" else optim.Adamax)
    errs = {}
    for flag, (adv, start, grads, end) in runs.items():
        p64 = [t.double().requires_grad_(True) for t in start]
        for p, gr in zip(p64, grads):
            p.grad = gr.double()
        parent = _parent(type(adv.optimizer))
        parent(p64, **{k: v for k, v in adv.optimizer.defaults.items() if k in ("lr", "betas", "eps", "weight_decay")}).step()
        if gan_type == "WGAN":
            with torch.no_grad():
                for p in p64:
                    p.clamp_(-1, 1)
            assert all(float(e.abs().max()) <= 1.0 for e in end)
        assert any(not torch.equal(e, s.double()) for e, s in zip(end, start))
        errs[flag] = [(float((e - p.detach()).abs().max()), _ulp(float(p.detach().abs().max()))) for e, p in zip(end, p64)]
    assert all(torch.equal(a, b) for a, b in zip(runs[False][1], runs[True][1]))          # the same start
    worst = max(on / (2.0 * off + ulp) for (on, ulp), (off, _) in zip(errs[True], errs[False]))
    print(f"{gan_type}: worst err / allowance {worst:.3f}")
    assert worst <= 1.0
