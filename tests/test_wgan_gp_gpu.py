"""The WGAN_GP term on the MI355X: the discriminator without BatchNorm (one autograd node over the HIP
kernels), `input_gradient` (a second node whose backward is the second-order pass), the penalty and its gradient to every
weight against float64 autograd of the restatement (tests/gradient_penalty_ref.py); `Adversarial.forward('WGAN_GP')` against
the same step written out here from the `ops` calls (bit for bit) and against float64; one epoch of the Trainer with
`--gradient_penalty --loss 1*Charb+0.005*WGAN_GP` against the loop written out, plus the command line in a child process.

The float64 reference takes every LeakyReLU's branch from an op-by-op replay of the product's forward (`_ops_forward` below,
whose logits must equal the node's bit for bit), so a value within rounding of zero cannot flip a branch between precisions.

Bound: relative L2 <= 2e-4 per tensor.  The same restatement in float32 on the CPU (same masks) is measured next to it; a
tensor on which that float32 reference itself is off by more than 5e-5 gets four times the reference's error instead.

The weights are scaled by 2.3 from their initial values so that the input gradient's norms are of order 0.1 .. 1 (they are
1e-4 at the default initialisation: ten layers of gain 0.45); each case asserts in float64 that | ||g_b|| - 1 | >= 0.1 for
every sample, so no comparison sits on the cancellation in (||g|| - 1)."""
import math
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import adacof_loss_ref as LR
import gradient_penalty_ref as GP
import train_batch_ref as TR
from conftest import PKG_DIR
from oracle import nets_cpu
from vfi_amd import ops
from vfi_amd.adacof import losses, utility
from vfi_amd.adacof.datareader import DBreader_Vimeo90k, TripletLoader
from vfi_amd.adacof.losses import adversarial, discriminator
from vfi_amd.adacof.models import Model
from vfi_amd.adacof.TestModule import Middlebury_other
from vfi_amd.adacof.trainer import Trainer

pytestmark = pytest.mark.gpu
RULE = 2e-4
REF32_LIMIT = 5e-5
GAIN = 2.3
SLOPE = GP.SLOPE
NB = GP.NB


def _seed(s):
    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)


def _scale(net, gain=GAIN):
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() > 1:
                p.mul_(gain)
    return net


def _params(net):
    sd = dict(net.named_parameters())
    return [sd[k] for k in GP.param_keys()]


# ---- the network written out from the ops calls -------------------------------------------------------------------------
def _ops_forward(params, x):
    """-> (logits, state): the eight blocks (convolution, then LeakyReLU as leaky_mask) and the classifier, call by call."""
    blocks, t = [], x.contiguous()
    for i, (_, _, stride) in enumerate(GP.BLOCKS):
        w = params[i]
        size = tuple(t.shape[2:])
        if stride == 2:
            w_eff, t_in = ops.stride2_weight(w), ops.phase_split(t)
        else:
            w_eff, t_in = w.detach(), t
        y = ops.conv2d(t_in, ops.PackedConv(w_eff), "zeros", None)
        out = ops.leaky_mask(y, y, SLOPE, out=y)
        blocks.append(dict(t_in=t_in, size=size, w_eff=w_eff, out=out, stride=stride))
        t = out
    flat = t.view(t.shape[0], -1)
    hid = ops.linear_forward(flat, params[NB], params[NB + 1], SLOPE)
    logits = ops.linear_forward(hid, params[NB + 2], params[NB + 3], 1.0)
    return logits, dict(blocks=blocks, flat=flat, hid=hid)


def _ops_backward(params, state, g, need_x, need_p=True):
    """First backward -> (dx or None, [dparam] or None, [u_1 .. u_10])."""
    grads = [None] * (NB + 4)
    g = g.contiguous()
    g_hid, grads[NB + 2], grads[NB + 3] = ops.linear_backward(state["hid"], params[NB + 2], None, 1.0, g, True, need_p, need_p)
    u_hid = ops.leaky_mask(g_hid, state["hid"], SLOPE, out=g_hid)
    g_flat, grads[NB], grads[NB + 1] = ops.linear_backward(state["flat"], params[NB], None, 1.0, u_hid, True, need_p, need_p)
    us = [u_hid, g]
    g_t = g_flat.view(state["blocks"][-1]["out"].shape)
    for i in range(NB - 1, -1, -1):
        s = state["blocks"][i]
        g_y = ops.leaky_mask(g_t, s["out"], SLOPE, out=g_t)
        us.insert(0, g_y)
        if need_p:
            dw, _ = ops.conv2d_backward_weight(s["t_in"], g_y, 3, "zeros", bias=False)
            grads[i] = ops.stride2_weight_gather(dw) if s["stride"] == 2 else dw
        if i == 0 and not need_x:
            g_t = None
            break
        g_in = ops.conv2d_backward_data(g_y, ops.packed_transposed(s["w_eff"]), "zeros")
        g_t = ops.phase_merge(g_in, s["size"]) if s["stride"] == 2 else g_in
    return g_t, (grads if need_p else None), us


def _ops_second_order(params, state, us, v):
    """The second-order pass from v_0 -> [dP/dparam], None for the four biases' two."""
    grads = [None] * (NB + 4)
    v = v.contiguous()
    for i in range(NB):
        s = state["blocks"][i]
        v_in = ops.phase_split(v) if s["stride"] == 2 else v
        dw, _ = ops.conv2d_backward_weight(v_in, us[i], 3, "zeros", bias=False)
        grads[i] = ops.stride2_weight_gather(dw) if s["stride"] == 2 else dw
        w = ops.conv2d(v_in, ops.PackedConv(s["w_eff"]), "zeros", None)
        v = ops.leaky_mask(w, s["out"], SLOPE, out=w)
    flat = v.view(v.shape[0], -1)
    grads[NB] = ops.linear_backward(flat, None, None, 1.0, us[NB], False, True, False)[1]
    w = ops.linear_forward(flat, params[NB], None, 1.0)
    v = ops.leaky_mask(w, state["hid"], SLOPE, out=w)
    grads[NB + 2] = ops.linear_backward(v, None, None, 1.0, us[NB + 1], False, True, False)[1]
    return grads


def _masks(state):
    return [s["out"] > 0 for s in state["blocks"]] + [state["hid"] > 0]


def _within_rule(name, got, ref64, ref32, worst):
    err, err32 = GP.rel(got, ref64), GP.rel(ref32, ref64)
    worst[name] = (err, err32)
    bound = RULE if err32 <= REF32_LIMIT else 4 * err32
    assert bool(torch.isfinite(got).all()) and err <= bound, (name, err, err32)


def _scalar_within_rule(name, got, ref64, ref32, worst):
    err, err32 = abs(float(got) - float(ref64)) / abs(float(ref64)), abs(float(ref32) - float(ref64)) / abs(float(ref64))
    worst[name] = (err, err32)
    assert math.isfinite(float(got)) and err <= (RULE if err32 <= REF32_LIMIT else 4 * err32), (name, err, err32)


# ---- the whole discriminator, input_gradient, the penalty ------------------------------------------------------------------
@pytest.mark.parametrize("patch,b", [(16, 4), (32, 2), (32, 3)])
def test_critic_input_gradient_and_penalty_against_float64(patch, b, device):
    _seed(patch + b)
    net = _scale(discriminator.Discriminator(GP.args(patch), 'WGAN_GP')).to(device)
    g = torch.Generator().manual_seed(b)
    x = torch.rand((b, 3, patch, patch), generator=g).to(device).requires_grad_(True)
    up = torch.randn((b, 1), generator=g).to(device)
    params = _params(net)
    logits = net(x)
    assert logits.shape == (b, 1) and type(logits.grad_fn).__name__.startswith("_CriticNode")
    (logits * up).sum().backward()
    with torch.no_grad():
        replay, state = _ops_forward(params, x.detach())
    assert torch.equal(replay, logits), "the replay is not the node's forward"
    masks = _masks(state)
    ref = GP.autograd_reference(params, x, masks, torch.float64, up)
    ref32 = GP.autograd_reference(params, x, masks, torch.float32, up)
    norms64 = ref["g"].flatten(1).norm(dim=1)
    assert float((norms64 - 1).abs().min()) >= 0.1, norms64          # precondition: off the cancellation
    worst = {}
    _within_rule("logits", logits, ref["logits"], ref32["logits"], worst)
    _within_rule("dx", x.grad, ref["dx"], ref32["dx"], worst)
    for k, p, r64, r32 in zip(GP.param_keys(), params, ref["dparams"], ref32["dparams"]):
        assert p.grad is not None and p.grad.shape == p.shape, k
        _within_rule("d " + k, p.grad, r64, r32, worst)

    net.zero_grad(set_to_none=True)
    grad = net.input_gradient(x.detach())
    assert grad.shape == x.shape and type(grad.grad_fn).__name__.startswith("_InputGradientNode")
    _within_rule("input_gradient", grad, ref["g"], ref32["g"], worst)
    value = adversarial.gradient_penalty(grad)
    assert type(value.grad_fn).__name__.startswith("_GradPenalty")
    _scalar_within_rule("penalty", value.detach(), ref["penalty"], ref32["penalty"], worst)
    value.backward()
    named = dict(net.named_parameters())
    for k, r64, r32 in zip(GP.weight_keys(), ref["dpenalty"], ref32["dpenalty"]):
        assert named[k].grad is not None and float(r64.norm()) > 0, k
        _within_rule("dP " + k, named[k].grad, r64, r32, worst)
    for k in ("classifier.0.bias", "classifier.2.bias"):            # the penalty sends nothing to the biases, nor to x
        assert named[k].grad is None or not bool(named[k].grad.any()), k
    top = sorted(worst.items(), key=lambda kv: -kv[1][0])[:4]
    print(f"WGAN_GP patch {patch} B {b}: norms {[round(float(v), 3) for v in norms64]}; logits {worst['logits'][0]:.2e}, "
          f"input_gradient {worst['input_gradient'][0]:.2e} (float32 CPU {worst['input_gradient'][1]:.2e}), penalty "
          f"{worst['penalty'][0]:.2e} ({worst['penalty'][1]:.2e}); worst tensors "
          + ", ".join(f"{k} {e:.2e} (float32 CPU {e32:.2e})" for k, (e, e32) in top))
    # the same bits on a second call, and through the replay written out from the ops calls
    assert torch.equal(net.input_gradient(x.detach()), grad)
    with torch.no_grad():
        g_ops, _, us = _ops_backward(params, state, torch.ones((b, 1), device=device), need_x=True, need_p=False)
        assert torch.equal(g_ops, grad)
        v0 = ops.grad_penalty_backward(grad.detach(), ops.grad_penalty_forward(grad.detach())[1], torch.ones((), device=device))
        for k, p, q in zip(GP.param_keys(), params, _ops_second_order(params, state, us, v0)):
            assert (q is None and p.grad is None) or torch.equal(p.grad, q), k


def test_frozen_and_the_other_faces(device):
    net = _scale(discriminator.Discriminator(GP.args(16), 'WGAN_GP')).to(device)
    x = torch.rand((1, 3, 16, 16), device=device, requires_grad=True)          # B = 1: there is no BatchNorm to refuse it
    with net.frozen():
        out = net(x)
        frozen_g = net.input_gradient(x)
    assert not frozen_g.requires_grad
    out.sum().backward()
    assert x.grad is not None and all(p.grad is None for p in net.parameters())
    full = net(x.detach())
    assert torch.equal(full, out) and type(full.grad_fn).__name__.startswith("_CriticNode")
    assert torch.equal(net.input_gradient(x), frozen_g) and torch.equal(frozen_g, x.grad)
    net.eval()
    assert "Node" not in type(net(x).grad_fn).__name__                          # eval mode: plain torch
    plain = net.input_gradient(x)                                               # torch's double backward
    assert "Node" not in type(plain.grad_fn).__name__ and GP.rel(plain, frozen_g) <= 1e-4
    net.train()
    with torch.no_grad():
        assert net(x).grad_fn is None


# ---- Adversarial.forward --------------------------------------------------------------------------------------------------
def _adversarial(patch, device, seed):
    _seed(seed)
    adv = adversarial.Adversarial(GP.args(patch), 'WGAN_GP')
    _scale(adv.discriminator)
    with torch.no_grad():                       # two values beyond [-1, 1]: WGAN's clamp would move them
        adv.discriminator.classifier[2].bias.fill_(1.5)
        adv.discriminator.features[0][0].weight[0, 0, 0, 0] = -1.7
    return adv.to(device)


def test_adversarial_forward_is_the_step_written_out(device):
    b, patch = 4, 16
    adv = _adversarial(patch, device, 3)
    start = [p.detach().clone() for p in _params(adv.discriminator)]
    g = torch.Generator().manual_seed(9)
    fake, real = (torch.rand((b, 3, patch, patch), generator=g).to(device) for _ in range(2))
    fake.requires_grad_(True)
    _seed(21)
    loss_g = adv(fake, real)
    got_grads = [None if p.grad is None else p.grad.clone() for p in _params(adv.discriminator)]
    loss_g.backward()
    assert isinstance(adv.loss, torch.Tensor) and adv.loss.dim() == 0 and adv.loss.is_cuda
    assert all((p.grad is None and q is None) or torch.equal(p.grad, q) for p, q in zip(_params(adv.discriminator), got_grads)), \
        "the frozen generator pass wrote a discriminator gradient"

    # the same step from the ops calls
    P = [p.clone().requires_grad_(True) for p in start]
    opt = torch.optim.Adam(P, betas=(0.0, 0.9), eps=1e-8, lr=1e-5)
    _seed(21)
    with torch.no_grad():
        (la, sa), (lb, sb) = _ops_forward(P, fake.detach()), _ops_forward(P, real)
        epsilon = torch.rand_like(fake)
        hat = ops.gp_mix(fake.detach(), real, epsilon)
        assert torch.equal(hat, fake.detach().mul(1 - epsilon) + real.mul(epsilon))
        _, sh = _ops_forward(P, hat)
        grad, _, us = _ops_backward(P, sh, torch.ones((b, 1), device=device), need_x=True, need_p=False)
        value, norms = ops.grad_penalty_forward(grad, 10.0)
    leaf_a, leaf_b, leaf_v = la.clone().requires_grad_(True), lb.clone().requires_grad_(True), value.clone().requires_grad_(True)
    loss_d = (leaf_a - leaf_b).mean() + leaf_v
    loss_d.backward()
    with torch.no_grad():
        _, ga, _ = _ops_backward(P, sa, leaf_a.grad, need_x=False)
        _, gb, _ = _ops_backward(P, sb, leaf_b.grad, need_x=False)
        gp = _ops_second_order(P, sh, us, ops.grad_penalty_backward(grad, norms, leaf_v.grad, 10.0))
    # autograd runs the nodes latest first: the penalty's, the real batch's, the fake batch's
    for p, u, v, w in zip(P, ga, gb, gp):
        p.grad = v + u if w is None else (w + v) + u
    assert float(adv.loss) == float(loss_d.detach())
    for k, p, q in zip(GP.param_keys(), got_grads, P):
        assert torch.equal(p, q.grad), k
    opt.step()
    for k, p, q, s in zip(GP.param_keys(), _params(adv.discriminator), P, start):
        assert torch.equal(p, q), k
        assert "bias" in k or not torch.equal(p, s), k
    assert adv.discriminator.classifier[2].bias.item() > 1.4 and adv.discriminator.features[0][0].weight[0, 0, 0, 0].item() < -1.6, \
        "a parameter was clamped"
    with torch.no_grad():
        lg, sg = _ops_forward(P, fake.detach())
    leaf_g = lg.clone().requires_grad_(True)
    want_g = -leaf_g.mean()
    want_g.backward()
    assert torch.equal(loss_g.detach(), want_g.detach())
    with torch.no_grad():
        gx, none, _ = _ops_backward(P, sg, leaf_g.grad, need_x=True, need_p=False)
    assert none is None and torch.equal(fake.grad, gx)

    # float64: loss_d and its gradient to every parameter, masks from the three replays, hat from the device's epsilon
    def loss_d_in(dtype):
        ps = [s.detach().cpu().to(dtype).requires_grad_(True) for s in start]
        cast = lambda t: t.detach().cpu().to(dtype)
        m = lambda st: [mk.cpu() for mk in _masks(st)]
        wass = (GP.forward(ps, cast(fake), m(sa)) - GP.forward(ps, cast(real), m(sb))).mean()
        gr = GP.input_gradient(ps, cast(hat), m(sh))
        total = wass + GP.penalty(gr)
        return total.detach(), torch.autograd.grad(total, ps, allow_unused=True), gr.detach().flatten(1).norm(dim=1)
    ld64, g64, norms64 = loss_d_in(torch.float64)
    ld32, g32, _ = loss_d_in(torch.float32)
    assert float((norms64 - 1).abs().min()) >= 0.1, norms64
    worst = {}
    _scalar_within_rule("loss_d", adv.loss, ld64, ld32, worst)
    for k, got, r64, r32 in zip(GP.param_keys(), got_grads, g64, g32):
        if r64 is None or float(r64.norm()) == 0:
            assert got is None or not bool(got.any()), k           # exactly 0 in float64: exactly 0 here
        else:
            _within_rule(k, got, r64, r32, worst)
    top = sorted(worst.items(), key=lambda kv: -kv[1][0])[:3]
    print("Adversarial.forward('WGAN_GP') vs float64: " + ", ".join(f"{k} {e:.2e} (float32 CPU {e32:.2e})" for k, (e, e32) in top))


# ---- the trainer --------------------------------------------------------------------------------------------------------
GP_LOSS = '1*Charb+0.005*WGAN_GP'


@pytest.fixture(scope="module")
def small_set(tmp_path_factory):
    """4 triplets of 40x56"""
    return TR.write_triplets(str(tmp_path_factory.mktemp("vimeo_small")), 4, 40, 56, seed=1, smooth=True)


@pytest.fixture(scope="module")
def middlebury(tmp_path_factory):
    return LR.write_middlebury(str(tmp_path_factory.mktemp("middlebury")), 40, 56, seed=3)


def _loader(root, device):
    return TripletLoader(DBreader_Vimeo90k(root, random_crop=(32, 32)), 2, shuffle=True, workers=2, device=device, rgb=True, lab=False)


def test_epoch_with_the_wgan_gp_term_is_the_manual_loop_bit_for_bit(small_set, middlebury, tmp_path, device):
    out = str(tmp_path / "out")
    args = GP.args(32, model="vfi_amd.adacof.models.adacofnet", kernel_size=5, dilation=1, out_dir=out, epochs=1, loss=GP_LOSS)
    state = nets_cpu.adacofnet_random_state_dict(12, kernel_size=5)
    model = Model(args)
    model.load(state)
    _seed(11)
    crit = losses.Loss(args)
    adv = crit.loss_module[1]
    assert isinstance(adv, adversarial.Adversarial) and adv.gan_type == 'WGAN_GP' and next(adv.parameters()).is_cuda
    twin = adversarial.Adversarial(args, 'WGAN_GP').to(device)
    twin.load_state_dict(adv.state_dict())
    d_start = [p.detach().clone() for p in adv.discriminator.parameters()]
    trainer = Trainer(args, _loader(small_set, device), Middlebury_other(*middlebury, device=device), model, crit)
    assert trainer.max_step == 2
    _seed(7)
    trainer.train()
    history = list(trainer.loss_history)
    trainer.test()
    trainer.close()
    assert os.path.exists(os.path.join(out, "checkpoint", "model_epoch001.pth"))

    ref = Model(args)
    ref.load(state)
    ref.train()
    opt = torch.optim.Adamax(ref.parameters(), lr=1e-3, betas=(0.9, 0.999), eps=1e-08, weight_decay=0)
    charb = utility.Module_CharbonnierLoss()
    _seed(7)
    manual, d_losses = [], []
    for batch in _loader(small_set, device):
        assert batch.rgb.shape == (3, 2, 3, 32, 32)
        opt.zero_grad()
        o = ref(batch.rgb_frame1, batch.rgb_frame2)
        value = sum([1.0 * charb(o["frame1"], batch.rgb_target), 0.005 * twin(o["frame1"], batch.rgb_target)])
        value.backward()
        opt.step()
        manual.append(float(value.detach()))
        d_losses.append(float(twin.loss))
    print("loss history:", history, "by hand:", manual, "discriminator losses:", d_losses)
    assert len(history) == 2 and all(math.isfinite(v) for v in history + d_losses) and history == manual
    for (k, p), (k2, q) in zip(model.named_parameters(), ref.named_parameters()):
        assert k == k2 and torch.equal(p, q), k
    changed = 0
    for p, q, s in zip(adv.discriminator.parameters(), twin.discriminator.parameters(), d_start):
        assert torch.equal(p, q)
        changed += not torch.equal(p, s)
    assert changed >= 2


def test_command_line_with_the_wgan_gp_term(small_set, middlebury, tmp_path, device):
    out = str(tmp_path / "cli")
    env = dict(os.environ)
    env["PYTHONPATH"] = PKG_DIR + os.pathsep + env.get("PYTHONPATH", "")
    base = [sys.executable, "-m", "vfi_amd.adacof.train", "--train", small_set, "--test_input", middlebury[0], "--gt", middlebury[1],
            "--out_dir", out, "--epochs", "1", "--batch_size", "2", "--patch_size", "32", "--workers", "2", "--gpu_id", "0",
            "--loss", GP_LOSS]
    r = subprocess.run(base + ["--gradient_penalty"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "0.005 * WGAN_GP" in r.stdout and "Train Epoch: [0/1]" in r.stdout and "Average: " in r.stdout
    assert os.path.exists(os.path.join(out, "checkpoint/model_epoch001.pth"))
    config = open(os.path.join(out, "config.txt")).read()
    assert "loss: " + GP_LOSS in config and "gradient_penalty: True" in config
