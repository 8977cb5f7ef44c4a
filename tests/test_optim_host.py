"""vfi_amd.optim without a device: on CPU parameters every class is its torch parent bit for bit,
the options the kernel does not restate are refused at construction, the wiring is off unless asked for, and the C entry
points answer bad requests before anything touches a device."""
import ctypes
import types

import pytest
import torch

import adversarial_ref as AR
from vfi_amd import _lib, ops, optim
from vfi_amd.adacof import utility
from vfi_amd.adacof.losses import adversarial

CLASSES = {
    "SGD": (optim.SGD, torch.optim.SGD, [dict(lr=0.1), dict(lr=0.1, momentum=0.9, weight_decay=1e-2),
                                         dict(lr=0.1, momentum=0.9, nesterov=True), dict(lr=0.1, momentum=0.5, dampening=0.3)]),
    "Adam": (optim.Adam, torch.optim.Adam, [dict(lr=1e-3), dict(lr=1e-5, betas=(0.0, 0.9), eps=1e-8),
                                            dict(lr=1e-3, weight_decay=1e-2)]),
    "Adamax": (optim.Adamax, torch.optim.Adamax, [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8),
                                                  dict(lr=1e-3, weight_decay=1e-2)]),
    "RMSprop": (optim.RMSprop, torch.optim.RMSprop, [dict(lr=1e-3, eps=1e-8), dict(lr=1e-3, weight_decay=1e-2, alpha=0.9)]),
}


def _params(seed, shapes=((7,), (3, 5), (2, 3, 3, 3))):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g).requires_grad_(True) for s in shapes]


def _set_grads(params, seed, skip=()):
    g = torch.Generator().manual_seed(seed)
    for i, p in enumerate(params):
        grad = torch.randn(p.shape, generator=g)
        p.grad = None if i in skip else grad


@pytest.mark.parametrize("name", sorted(CLASSES))
def test_cpu_step_is_the_parent_class_bit_for_bit(name):
    cls, parent, options = CLASSES[name]
    assert issubclass(cls, parent) and cls.__name__ == parent.__name__
    for kw in options:
        a, b = _params(1), _params(1)
        oa, ob = cls(a, **kw), parent(b, **kw)
        for step in range(3):
            skip = (1,) if step == 1 else ()                  # one step in which a parameter has no grad
            _set_grads(a, 10 + step, skip)
            _set_grads(b, 10 + step, skip)
            versions = [p._version for p in a]
            oa.step()
            ob.step()
            assert all(torch.equal(x, y) for x, y in zip(a, b)), (name, kw, step)
            assert all(p._version > v for i, (p, v) in enumerate(zip(a, versions)) if i not in skip)
        sa, sb = oa.state_dict(), ob.state_dict()
        assert sa["param_groups"] == sb["param_groups"] and sa["state"].keys() == sb["state"].keys()
        for k in sa["state"]:
            assert sa["state"][k].keys() == sb["state"][k].keys()
            assert all(torch.equal(torch.as_tensor(sa["state"][k][n]), torch.as_tensor(sb["state"][k][n])) for n in sa["state"][k])


def test_cpu_step_with_clamp_and_closure():
    a, b = _params(2), _params(2)
    oa, ob = optim.Adam(a, lr=0.5), torch.optim.Adam(b, lr=0.5)
    _set_grads(a, 3)
    _set_grads(b, 3)
    calls = []
    assert oa.step(lambda: calls.append(1) or torch.tensor(4.0), clamp=(-0.25, 0.25)) == 4.0 and calls == [1]
    ob.step()
    assert any(float(p.detach().abs().max()) > 0.25 for p in b)
    assert all(torch.equal(x, y.detach().clamp(-0.25, 0.25)) for x, y in zip(a, b))


def test_step_hooks_run_once():
    a = _params(4)
    opt = optim.Adamax(a, lr=1e-3)
    seen = []
    opt.register_step_pre_hook(lambda *args: seen.append("pre"))
    opt.register_step_post_hook(lambda *args: seen.append("post"))
    torch.optim.Adamax(_params(4), lr=1e-3)                   # the parent's step is wrapped by its own instances too
    _set_grads(a, 5)
    opt.step()
    assert seen == ["pre", "post"]


def test_refused_options_raise():
    p = _params(6)
    for cls, kw in ((optim.Adam, dict(amsgrad=True)), (optim.Adam, dict(maximize=True)), (optim.Adam, dict(capturable=True)),
                    (optim.Adam, dict(differentiable=True)), (optim.Adam, dict(decoupled_weight_decay=True)),
                    (optim.Adam, dict(fused=True)), (optim.Adam, dict(lr=torch.tensor(1e-3))),
                    (optim.Adamax, dict(maximize=True)), (optim.Adamax, dict(capturable=True)),
                    (optim.Adamax, dict(differentiable=True)),
                    (optim.RMSprop, dict(centered=True)), (optim.RMSprop, dict(momentum=0.9)), (optim.RMSprop, dict(maximize=True)),
                    (optim.RMSprop, dict(capturable=True)), (optim.RMSprop, dict(differentiable=True)),
                    (optim.SGD, dict(maximize=True)), (optim.SGD, dict(differentiable=True)), (optim.SGD, dict(fused=True))):
        with pytest.raises(ValueError, match="not implemented on the device"):
            cls(p, **kw)
    opt = optim.Adam(p[:1])
    with pytest.raises(ValueError, match="amsgrad"):
        opt.add_param_group(dict(params=p[1:], amsgrad=True))


def test_refused_options_raise_when_loaded():
    p = _params(6)
    sd = torch.optim.Adam(p, amsgrad=True).state_dict()
    with pytest.raises(ValueError, match="amsgrad"):
        optim.Adam(_params(6)).load_state_dict(sd)
    opt = optim.Adam(_params(6))
    opt.load_state_dict(torch.optim.Adam(p, lr=0.25).state_dict())
    assert opt.param_groups[0]["lr"] == 0.25


def test_make_optimizer_follows_the_flag():
    net = torch.nn.Linear(3, 2)
    for name, parent in (("SGD", torch.optim.SGD), ("ADAM", torch.optim.Adam), ("ADAMax", torch.optim.Adamax),
                         ("RMSprop", torch.optim.RMSprop)):
        off = utility.make_optimizer(AR.args(16, optimizer=name), net)
        assert type(off) is parent
        assert type(utility.make_optimizer(AR.args(16, optimizer=name, device_optimizer=False), net)) is parent
        on = utility.make_optimizer(AR.args(16, optimizer=name, device_optimizer=True, lr=3e-4, weight_decay=1e-3), net)
        assert type(on) is getattr(optim, parent.__name__) and isinstance(on, parent)
        want = parent(net.parameters(), lr=3e-4, weight_decay=1e-3, **utility._OPTIMIZERS[name][1])
        assert on.defaults == want.defaults


def test_adversarial_follows_the_flag():
    gp = adversarial.Adversarial(AR.args(16, gradient_penalty=True), 'WGAN_GP')
    assert type(gp.optimizer) is torch.optim.Adam and not gp.device_optimizer
    assert type(adversarial.Adversarial(AR.args(16), 'WGAN').optimizer) is torch.optim.Adamax
    gp = adversarial.Adversarial(AR.args(16, gradient_penalty=True, device_optimizer=True), 'WGAN_GP')
    assert type(gp.optimizer) is optim.Adam and gp.optimizer.defaults["betas"] == (0.0, 0.9) and gp.optimizer.defaults["lr"] == 1e-5
    assert type(adversarial.Adversarial(AR.args(16, device_optimizer=True), 'WGAN').optimizer) is optim.Adamax


def test_adversarial_wgan_on_the_cpu_is_unchanged_by_the_flag():
    """On CPU tensors the device class is its parent and the clamp is the torch loop: the same bits with the flag on and off."""
    out = []
    for flag in (False, True):
        torch.manual_seed(5)
        adv = adversarial.Adversarial(AR.args(16, device_optimizer=flag), 'WGAN')
        with torch.no_grad():
            adv.discriminator.classifier[2].bias.fill_(1.5)
        g = torch.Generator().manual_seed(6)
        fake, real = torch.rand((2, 3, 16, 16), generator=g), torch.rand((2, 3, 16, 16), generator=g)
        adv(fake, real)
        out.append([p.detach().clone() for p in adv.discriminator.parameters()])
    assert all(torch.equal(x, y) for x, y in zip(*out))
    assert float(out[1][-1].max()) == 1.0


def test_trainers_build_the_device_adam_under_the_flag(monkeypatch, tmp_path):
    from vfi_amd.fusion_net import trainer as fusion_trainer
    from vfi_amd.train import trainer as phase_trainer
    net = torch.nn.Linear(3, 2)
    net.fine_tune = lambda *a, **k: None
    pyr = types.SimpleNamespace(device=torch.device("cpu"))
    for flag, want in ((None, torch.optim.Adam), (False, torch.optim.Adam), (True, optim.Adam)):
        extra = {} if flag is None else {"device_optimizer": flag}
        t = fusion_trainer.Trainer(types.SimpleNamespace(**extra), [], net, None, None, pyr, out_dir=str(tmp_path))
        assert type(t.optimizer) is want
        t.logfile.close()
        t = phase_trainer.Trainer(types.SimpleNamespace(mode="phase", high_level=False, **extra), [], net, pyr, out_dir=str(tmp_path))
        assert type(t.optimizer) is want
        t.logfile.close()


def test_command_lines_accept_the_flag():
    from vfi_amd.adacof import train as adacof_train
    from vfi_amd.fusion_net import train as fusion_train
    from vfi_amd.train import train as phase_train
    for m in (adacof_train, fusion_train, phase_train):
        assert m.parser.parse_args([]).device_optimizer is False
        assert m.parser.parse_args(["--device_optimizer"]).device_optimizer is True


# ---- the C entry points ---------------------------------------------------------------------------------------------------
def _hyper(**kw):
    base = dict(lr=1e-3, beta1=0.9, beta2=0.999, alpha=0.99, eps=1e-8, bias_correction1=0.1, bias_correction2=0.001)
    base.update(kw)
    return _lib.OptimHyper(**base)


def _step(kind, recs, count, hyper):
    return _lib.lib().vfi_optim_step(kind, ctypes.addressof(recs) if recs is not None else None, count,
                                     ctypes.addressof(hyper) if hyper is not None else None, None)


def test_limits_entry():
    chunk, tensors, chunks, max_numel = ops.optim_limits()
    assert chunk > 0 and chunk % 4 == 0 and tensors > 0 and chunks >= tensors and max_numel > 2 ** 31
    assert _lib.lib().vfi_optim_limits(None, None, None, None) == -1


def test_step_entry_validates_without_a_device():
    INVALID, UNSUPPORTED = -1, -4
    _, _, _, max_numel = ops.optim_limits()
    some = 4096                                             # never dereferenced: every call below is refused on the host
    good = lambda n=8: _lib.OptimTensor(param=some, grad=some, state0=some, state1=some, numel=n)
    one = (_lib.OptimTensor * 1)(good())
    h = _hyper()
    assert _step(1, None, 1, h) == INVALID and _step(1, one, 1, None) == INVALID
    assert _step(1, one, 0, h) == INVALID and _step(1, one, -3, h) == INVALID
    assert _step(4, one, 1, h) == INVALID and _step(-1, one, 1, h) == INVALID
    assert b"unknown kind" in _lib.lib().vfi_last_error()
    for bad in (dict(param=None), dict(grad=None), dict(numel=0), dict(numel=-5), dict(state0=None), dict(state1=None)):
        rec = good()
        for k, v in bad.items():
            setattr(rec, k, v)
        two = (_lib.OptimTensor * 2)(good(), rec)
        assert _step(1, two, 2, h) == INVALID, bad
        assert _step(2, two, 2, h) == INVALID, bad
    # state the kind does not use may be null -- but then the grad-less record is still refused
    rec = good()
    rec.state1 = None
    rec.grad = None
    assert _step(3, (_lib.OptimTensor * 1)(rec), 1, h) == INVALID
    rec = good()
    rec.state0 = None
    assert _step(0, (_lib.OptimTensor * 1)(rec), 1, _hyper(momentum=0.9)) == INVALID      # SGD with momentum needs its buffer
    big = (_lib.OptimTensor * 2)(good(), good(max_numel + 1))
    for kind in range(4):
        assert _step(kind, big, 2, h) == UNSUPPORTED
    assert b"numel" in _lib.lib().vfi_last_error()
    assert _step(1, one, 1, _hyper(bias_correction1=0.0)) == INVALID
    assert _step(1, one, 1, _hyper(beta2=1.0)) == INVALID
    assert _step(0, one, 1, _hyper(nesterov=1, momentum=0.0)) == INVALID
    assert _step(1, one, 1, _hyper(has_clamp=1, clamp_min=1.0, clamp_max=-1.0)) == INVALID


def test_ops_optim_step_has_no_cpu_path():
    p = _params(8)
    with pytest.raises((_lib.VfiLibraryError, RuntimeError, AssertionError)):
        ops.optim_step("adam", p, [torch.zeros_like(x) for x in p], [torch.zeros_like(x) for x in p],
                       [torch.zeros_like(x) for x in p], lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
