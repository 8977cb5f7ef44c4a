"""Training helpers of the AdaCoF network -- mirror of reference src/adacof/utility.py (same names and signatures).

`CharbonnierFunc` / `Module_CharbonnierLoss` (utility.py:67-77) run as one HIP autograd node (a fixed-order two-stage
reduction forward, one streaming pass backward) when they are given HIP tensors of which one requires grad, so the
reference loss `1*Charb` on `output['frame1']` stays off torch's elementwise kernels; any other argument (CPU tensors,
float64, nothing requiring grad) takes the plain torch expression (`_on_hip` decides, for the MSE / L1 nodes of
`losses/__init__.py` too).  The trainer's `Loss`, its VGG term and its GAN terms (`losses/adversarial.py`,
whose discriminator takes its optimiser and scheduler from `make_optimizer` / `make_scheduler` here) are in `losses/`.
"""
import torch
import torch.nn as nn
import torch.optim as optim
import torch.optim.lr_scheduler as lrs

from .. import ops

CHANNEL_MEANS = (0.4631, 0.4352, 0.3990)     # utility.py:86-87


class _Charbonnier(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, epsilon):
        a = a.contiguous()
        b = b.contiguous() if b is not None else None
        ctx.epsilon = epsilon
        ctx.save_for_backward(a, b)
        return ops.charbonnier_forward(a, b, epsilon)

    @staticmethod
    def backward(ctx, upstream):
        a, b = ctx.saved_tensors
        need_a, need_b = ctx.needs_input_grad[0], b is not None and ctx.needs_input_grad[1]
        ga, gb = ops.charbonnier_backward(a, b, upstream.contiguous(), ctx.epsilon, need_a=need_a, need_b=need_b)
        return ga, gb, None


def _on_hip(*tensors):
    ts = [t for t in tensors if t is not None]
    return (torch.is_grad_enabled() and all(t.is_cuda and t.dtype == torch.float32 for t in ts)
            and any(t.requires_grad for t in ts))


def _charbonnier(a, b, epsilon):
    if b is not None and a.shape != b.shape:
        a, b = torch.broadcast_tensors(a, b)
    if _on_hip(a, b):
        return _Charbonnier.apply(a, b, float(epsilon))
    d = a if b is None else a - b
    return torch.mean(torch.sqrt(d ** 2 + epsilon ** 2))


def CharbonnierFunc(data, epsilon=0.001):
    """mean(sqrt(data^2 + epsilon^2)) (utility.py:67-68)."""
    return _charbonnier(data, None, epsilon)


class Module_CharbonnierLoss(nn.Module):
    """mean(sqrt((output - gt)^2 + epsilon^2)) (utility.py:71-77)."""

    def __init__(self, epsilon=0.001):
        super().__init__()
        self.epsilon = epsilon

    def forward(self, output, gt):
        return _charbonnier(output, gt, self.epsilon)


def moduleNormalize(frame):
    """Subtracts the channel means (utility.py:86-87)."""
    return frame - torch.tensor(CHANNEL_MEANS, dtype=frame.dtype, device=frame.device).view(1, 3, 1, 1)


_OPTIMIZERS = {"SGD": (optim.SGD, {"momentum": 0.9}),
               "ADAM": (optim.Adam, {"betas": (0.9, 0.999), "eps": 1e-08}),
               "ADAMax": (optim.Adamax, {"betas": (0.9, 0.999), "eps": 1e-08}),
               "RMSprop": (optim.RMSprop, {"eps": 1e-08})}


def make_optimizer(args, my_model):
    """args.optimizer in SGD | ADAM | ADAMax | RMSprop with args.lr and args.weight_decay over the parameters that
    require grad (utility.py:19-44).  With a true args.device_optimizer (absent = false) it is vfi_amd.optim's subclass of
    that torch class."""
    cls, kwargs = _OPTIMIZERS[args.optimizer]
    if getattr(args, 'device_optimizer', False):      # the same class with its step on the device (vfi_amd/optim.py)
        from .. import optim as device_optim
        cls = getattr(device_optim, cls.__name__)
    trainable = [p for p in my_model.parameters() if p.requires_grad]
    return cls(trainable, lr=args.lr, weight_decay=args.weight_decay, **kwargs)


def make_scheduler(args, my_optimizer):
    """args.decay_type 'step' (StepLR every args.lr_decay) or 'step_a_b_...' (MultiStepLR at a, b, ...), gamma
    args.gamma (utility.py:47-64)."""
    if args.decay_type == "step":
        return lrs.StepLR(my_optimizer, step_size=args.lr_decay, gamma=args.gamma)
    if "step" in args.decay_type:
        milestones = [int(x) for x in args.decay_type.split("_")[1:]]
        return lrs.MultiStepLR(my_optimizer, milestones=milestones, gamma=args.gamma)
    raise ValueError(f"unknown decay_type {args.decay_type!r}")
