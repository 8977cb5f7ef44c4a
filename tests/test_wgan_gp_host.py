"""The WGAN_GP term without a GPU: the no-BatchNorm discriminator's state-dict layout, the `Loss`
grammar with and without `args.gradient_penalty`, the refusals, the new entries' error statuses, the written-out first
backward / second-order chain of tests/gradient_penalty_ref.py against torch's double backward of the plain module in
float64, and `Adversarial.forward('WGAN_GP')` on the CPU in float64 against the reference's step written out.

Bounds.  The chain and torch's double backward are the same sums in float64 in another order: 1e-11 relative L2 per weight
gradient (measured below 1e-15) -- two mutants of the chain (the mask left off the tangent; u_{k+1} for u_k) miss it by
ten orders of magnitude.  The step written out runs the same torch operations as the module: 1e-12."""
import copy
import types

import pytest
import torch

import adversarial_ref as AR
import gradient_penalty_ref as GP
from vfi_amd import _lib
from vfi_amd.adacof import losses
from vfi_amd.adacof.losses import adversarial, discriminator


def _net(patch, seed=0):
    torch.manual_seed(seed)
    return discriminator.Discriminator(GP.args(patch), 'WGAN_GP')


@pytest.mark.parametrize("patch", [16, 32, 256])
def test_state_dict_is_the_reference_layout(patch):
    if patch == 256:
        with torch.device("meta"):
            net = discriminator.Discriminator(GP.args(patch), 'WGAN_GP')
    else:
        net = _net(patch)
    want = GP.layout(patch)
    got = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    assert got == want and list(got) == list(want) == GP.param_keys()
    assert [n for n, _ in net.named_parameters()] == GP.param_keys()
    assert net.classifier[0].in_features == 512 * (patch // 16) ** 2
    for i, (_, _, stride) in enumerate(GP.BLOCKS):
        blk = net.features[i]
        assert len(blk) == 2 and isinstance(blk[0], torch.nn.Conv2d) and blk[0].bias is None and blk[0].stride == (stride, stride)
        assert isinstance(blk[1], torch.nn.LeakyReLU) and blk[1].negative_slope == 0.2
    assert not any(isinstance(m, torch.nn.BatchNorm2d) for m in net.modules())


def test_loss_grammar_with_the_flag(capsys):
    a = GP.args(16, loss='1*Charb+0.005*WGAN_GP+0.5*WGAN+0.01*g_Spatial')
    crit = losses.Loss(a)
    assert [l['type'] for l in crit.loss] == ['Charb', 'WGAN_GP', 'WGAN'] and [l['weight'] for l in crit.loss] == [1, 0.005, 0.5]
    assert crit.regularize == [{'type': 'g_Spatial', 'weight': 0.01}]
    gp, wgan = list(crit.loss_module)[1:]
    assert isinstance(gp, adversarial.Adversarial) and gp.gan_type == 'WGAN_GP' and gp.gan_k == 1
    assert isinstance(gp.discriminator, discriminator.Discriminator) and not gp.discriminator._bn and wgan.discriminator._bn
    opt = gp.optimizer
    assert type(opt) is torch.optim.Adam and opt.defaults['betas'] == (0, 0.9) and opt.defaults['eps'] == 1e-8
    assert opt.defaults['lr'] == 1e-5 and opt.defaults['weight_decay'] == 0
    assert gp.scheduler.step_size == 20 and gp.scheduler.gamma == 0.5 and gp.scheduler.optimizer is opt
    assert isinstance(wgan.optimizer, torch.optim.Adamax)               # the other types keep args.optimizer
    assert "0.005 * WGAN_GP" in capsys.readouterr().out
    assert adversarial.TYPES == ('GAN', 'WGAN', 'FI_GAN') and adversarial.built_types(a) == adversarial.TYPES + ('WGAN_GP',)
    assert adversarial.built_types(AR.args(16)) == adversarial.TYPES


def test_refusals_without_the_flag():
    for flag in ({}, {"gradient_penalty": False}):
        for string in ('1*WGAN_GP', '1*Charb+0.005*WGAN_GP'):
            for a in (types.SimpleNamespace(loss=string, **flag), AR.args(32, loss=string, **flag)):
                with pytest.raises(NotImplementedError, match='discriminator is not built'):
                    losses.Loss(a)
        with pytest.raises(NotImplementedError, match="only GAN, WGAN, FI_GAN have a discriminator built"):
            adversarial.Adversarial(AR.args(32, **flag), 'WGAN_GP')
        with pytest.raises(NotImplementedError, match="gan_type 'WGAN_GP'"):
            discriminator.Discriminator(AR.args(32, **flag), 'WGAN_GP')
    with pytest.raises(NotImplementedError, match='patch_size'):        # the flag does not size the classifier
        losses.Loss(types.SimpleNamespace(loss='1*WGAN_GP', gradient_penalty=True))


def test_t_wgan_gp_is_refused_with_and_without_the_flag():
    for a in (AR.args(32, loss='1*Charb+0.01*T_WGAN_GP'), GP.args(32, loss='1*Charb+0.01*T_WGAN_GP')):
        with pytest.raises(NotImplementedError, match='discriminator is not built'):
            losses.Loss(a)
        with pytest.raises(NotImplementedError):
            adversarial.Adversarial(a, 'T_WGAN_GP')
    assert not hasattr(discriminator, 'Temporal_Discriminator')


def test_library_refusals_need_no_device():
    h = _lib.lib()
    one = 16
    ok_mask = (one, 4, one, 4, one, 4, 1, 4)
    assert h.vfi_leaky_mask(None, 4, one, 4, one, 4, 1, 4, 0.2, None) == -1
    assert h.vfi_leaky_mask(one, 4, None, 4, one, 4, 1, 4, 0.2, None) == -1
    assert h.vfi_leaky_mask(one, 4, one, 4, None, 4, 1, 4, 0.2, None) == -1
    assert h.vfi_leaky_mask(one, 4, one, 4, one, 4, 0, 4, 0.2, None) == -1 and h.vfi_leaky_mask(one, 4, one, 4, one, 4, 1, 0, 0.2, None) == -1
    for slope in (0.0, -0.2):
        assert h.vfi_leaky_mask(*ok_mask, slope, None) == -1
        assert b"slope" in h.vfi_last_error()
    for k in range(4):
        ptrs = [one] * 4
        ptrs[k] = None
        assert h.vfi_gp_mix(ptrs[0], 4, ptrs[1], 4, ptrs[2], 4, ptrs[3], 4, 1, 4, None) == -1
        assert h.vfi_grad_penalty_backward(ptrs[0], 4, ptrs[1], ptrs[2], ptrs[3], 4, 1, 4, 10.0, None) == -1
    for n, count in ((0, 4), (1, 0), (-1, 4), (1, -4)):
        assert h.vfi_gp_mix(one, 4, one, 4, one, 4, one, 4, n, count, None) == -1
        assert h.vfi_grad_penalty_forward(one, 4, one, one, n, count, 10.0, None) == -1
        assert h.vfi_grad_penalty_backward(one, 4, one, one, one, 4, n, count, 10.0, None) == -1
    for k in range(3):
        ptrs = [one] * 3
        ptrs[k] = None
        assert h.vfi_grad_penalty_forward(ptrs[0], 4, ptrs[1], ptrs[2], 1, 4, 10.0, None) == -1


# ---- the identity ---------------------------------------------------------------------------------------------------------
def _double_backward_of_the_module(patch, b, seed):
    net = _net(patch, seed).double()
    g = torch.Generator().manual_seed(patch * 10 + b)
    x = torch.rand((b, 3, patch, patch), generator=g, dtype=torch.float64)
    grad = net.input_gradient(x)                    # CPU: autograd.grad(create_graph=True) through torch's own modules
    value = GP.penalty(grad)
    named = dict(net.named_parameters())
    got = torch.autograd.grad(value, [named[k] for k in GP.param_keys()], allow_unused=True)
    params = [named[k].detach() for k in GP.param_keys()]
    masks = []
    logits = GP.forward(params, x, keep=masks)
    assert GP.rel(logits, net(x)) <= 1e-13
    return params, x, masks, grad.detach(), value.detach(), dict(zip(GP.param_keys(), got))


@pytest.mark.parametrize("patch,b", [(16, 3), (32, 1)])
def test_written_out_chain_is_torchs_double_backward(patch, b):
    params, x, masks, grad, value, want = _double_backward_of_the_module(patch, b, seed=patch + b)
    g, p, got = GP.chain(params, x, masks)
    assert GP.rel(g, grad) <= 1e-11 and abs(float(p) - float(value)) <= 1e-11 * abs(float(value))
    worst = {}
    for k in GP.weight_keys():
        worst[k] = GP.rel(got[k], want[k])
        assert float(want[k].norm()) > 0 and worst[k] <= 1e-11, (k, worst[k])
    print(f"chain vs double backward, patch {patch} B {b}: worst {max(worst.values()):.2e}")
    bias1 = want["classifier.0.bias"]
    assert bias1 is not None and bias1.shape == (1024,) and not bool(bias1.any())          # exactly 0
    assert not bool(got["classifier.0.bias"].any()) and not bool(got["classifier.2.bias"].any())
    assert want["classifier.2.bias"] is None or not bool(want["classifier.2.bias"].any())
    # the float64 comparison sees the two mutants of section 28
    for flags in (dict(drop_tangent_mask=True), dict(shift_u=True)):
        _, _, bad = GP.chain(params, x, masks, **flags)
        assert max(GP.rel(bad[k], want[k]) for k in GP.weight_keys()) > 1e-3, flags


def test_input_gradient_sends_nothing_to_x():
    net = _net(16, 1).double()
    x = torch.rand((2, 3, 16, 16), dtype=torch.float64, requires_grad=True)
    g = net.input_gradient(x)
    assert g.shape == x.shape and g.requires_grad
    GP.penalty(g).backward()
    assert x.grad is None and all(p.grad is not None for k, p in net.named_parameters() if k != "classifier.2.bias")


# ---- Adversarial.forward --------------------------------------------------------------------------------------------------
def test_adversarial_forward_on_the_cpu_is_the_reference_step():
    b, patch = 3, 16
    torch.manual_seed(5)
    adv = adversarial.Adversarial(GP.args(patch), 'WGAN_GP').double()
    twin = copy.deepcopy(adv.discriminator)
    before = {k: v.clone() for k, v in adv.discriminator.state_dict().items()}
    g = torch.Generator().manual_seed(6)
    fake = torch.rand((b, 3, patch, patch), generator=g, dtype=torch.float64).requires_grad_(True)
    real = torch.rand((b, 3, patch, patch), generator=g, dtype=torch.float64)
    torch.manual_seed(77)
    loss_g = adv(fake, real)
    assert isinstance(adv.loss, torch.Tensor) and adv.loss.dim() == 0
    got_grads = {k: p.grad.clone() for k, p in adv.discriminator.named_parameters()}

    # reference src/adacof/losses/adversarial.py:43-44,55-68,71-73,93-94
    opt = torch.optim.Adam(twin.parameters(), betas=(0.0, 0.9), eps=1e-8, lr=1e-5)
    torch.manual_seed(77)
    fake_detach = fake.detach()
    opt.zero_grad()
    loss_d = (twin(fake_detach) - twin(real)).mean()
    epsilon = torch.rand_like(fake)
    hat = fake_detach.mul(1 - epsilon) + real.mul(epsilon)
    hat.requires_grad = True
    gradients = torch.autograd.grad(outputs=twin(hat).sum(), inputs=hat, retain_graph=True, create_graph=True, only_inputs=True)[0]
    gradient_norm = gradients.view(gradients.size(0), -1).norm(2, dim=1)
    loss_d = loss_d + 10 * gradient_norm.sub(1).pow(2).mean()
    loss_d.backward()
    assert abs(float(adv.loss) - float(loss_d)) <= 1e-12 * abs(float(loss_d))
    assert float(gradient_norm.sub(1).abs().min()) > 1e-3          # the penalty is live in this comparison
    for k, p in twin.named_parameters():
        assert GP.rel(got_grads[k], p.grad) <= 1e-12, k
    opt.step()
    want_g = -twin(fake).mean()
    assert abs(float(loss_g) - float(want_g)) <= 1e-12 * abs(float(want_g))
    after = adv.discriminator.state_dict()
    for k, p in twin.state_dict().items():
        assert GP.rel(after[k], p) <= 1e-12, k
        # (the biases get nothing from the penalty, and from the Wasserstein term the difference of two batch means of the
        # hidden layer's masks -- 0 for the last bias, and for the first one wherever the masks agree: Adam leaves those)
        assert "bias" in k or not torch.equal(after[k], before[k]), k
    assert all(float(p.detach().abs().max()) > 0 for p in adv.discriminator.parameters() if p.dim() > 1)
    loss_g.backward()
    assert fake.grad is not None and float(fake.grad.abs().sum()) > 0
