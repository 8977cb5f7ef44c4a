"""Optimisers whose step runs on the device: `SGD`, `Adam`, `Adamax` and `RMSprop`, each a subclass of the `torch.optim`
class of the same name with the same constructor.  DESIGN.md section 29.

`step(closure=None, clamp=None)` updates every parameter that has a grad in one multi-tensor HIP pass per set of parameters
that share hyper-parameters and a step count (`ops.optim_step`, csrc/vfi_optim.hip), with `clamp=(lo, hi)` applied to the
new values in the same pass.  The state lives under torch's own keys and layouts (`step` as the parent keeps it, `exp_avg`,
`exp_avg_sq`, `exp_inf`, `square_avg`, `momentum_buffer`), so `state_dict()` / `load_state_dict()` interchange with the
parent class and a run may change class at a checkpoint; `lr` is read from the param group at every step, so the
schedulers work unchanged.  A parameter without a grad is skipped and its step count stays.

The kernel writes through raw pointers.  torch's version counters therefore do not move by themselves, and
`PackedModule.packed()` (nn_util.py) keys its packed weights on them: `step` bumps the counter of every parameter it wrote
with one `torch.autograd.graph.increment_version` call, so the packs rebuild at the next forward.

The kernel takes contiguous float32 HIP parameters with contiguous dense float32 grads.  If a parameter that has a grad is
anything else (CPU, another dtype, a strided view), the WHOLE call is the parent class's step followed by the clamp as
a torch loop over the parameters that had a grad: on the CPU the result is torch's, bit for bit.  Options the kernel does
not restate are refused at construction, not ignored: amsgrad, maximize, capturable, differentiable,
decoupled_weight_decay, fused, tensor-valued lr or betas, centred RMSprop and RMSprop with momentum."""
import torch
from torch.optim.optimizer import _get_scalar_dtype

from . import ops

_REFUSED = ("amsgrad", "maximize", "capturable", "differentiable", "decoupled_weight_decay", "fused", "centered")


def _eligible(t):
    return t.is_cuda and t.dtype is torch.float32 and t.layout is torch.strided and t.is_contiguous()


class _DeviceStep:
    """The step the four classes share.  `_kind` names the kernel; a class says which state a group keeps (`_states`, in
    the kernel's order), what distinguishes the sets of one group (`_count`) and the kernel's scalars (`_hyper`)."""
    _kind = None

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._check_options()

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        self._check_options()

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._check_options()      # the loaded param groups bring their own options

    def _check_options(self):
        name = f"vfi_amd.optim.{type(self).__name__}"
        for group in self.param_groups:
            for option in _REFUSED:
                if group.get(option):
                    raise ValueError(f"{name}: {option} is not implemented on the device")
            if self._kind == "rmsprop" and group["momentum"] != 0:
                raise ValueError(f"{name}: momentum is not implemented on the device")
            if any(isinstance(v, torch.Tensor) for v in (group["lr"], *group.get("betas", ()))):
                raise ValueError(f"{name}: a tensor lr or beta is not implemented on the device")

    def _states(self, group):
        raise NotImplementedError

    def _hyper(self, group, count):
        raise NotImplementedError

    def _count(self, group, state):
        """What the update of a parameter depends on besides its group: the step count after this update."""
        return float(state["step"]) + 1.0

    def _begin(self, group, count, params):
        """Just before the launch of a set."""

    def _abort(self, group, count, params):
        """The launch of a set raised: undo _begin."""

    def _advance(self, group, count, params):
        for p in params:
            self.state[p]["step"] += 1

    def _init_state(self, group, state, p):
        if len(state) == 0:
            state["step"] = torch.tensor(0.0, dtype=_get_scalar_dtype())     # on the host, as the parent keeps it
            for key in self._states(group):
                state[key] = torch.zeros_like(p, memory_format=torch.preserve_format)

    def _parent_step(self):
        mro = type(self).__mro__
        step = mro[mro.index(_DeviceStep) + 1].step
        if getattr(step, "hooked", False):     # wrapped by Optimizer.__init__ to run the step hooks, which our own wrapper did
            step = step.__wrapped__
        step(self)

    def _sets(self):
        """-> (parameters to step, [(group, count, params)], the params of a set on one device), or None where a parameter with a grad cannot go through the
        kernel.  Creates missing state as the parent class does; advances nothing."""
        stepped, sets = [], []
        for group in self.param_groups:
            keys, by_count = self._states(group), {}
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if not (_eligible(p) and _eligible(g) and g.device == p.device):
                    return None
                state = self.state[p] if keys else {}      # (SGD without momentum keeps none, as the parent)
                self._init_state(group, state, p)
                for key in keys:
                    s = state.get(key)
                    if s is not None and not (_eligible(s) and s.shape == p.shape and s.device == p.device):
                        return None
                by_count.setdefault((self._count(group, state), p.device), []).append(p)      # one device per launch
                stepped.append(p)
            sets.extend((group, count, params) for (count, _), params in by_count.items())
        return stepped, sets

    @torch.no_grad()
    def step(self, closure=None, clamp=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        found = self._sets()
        if found is None:
            stepped = [p for group in self.param_groups for p in group["params"] if p.grad is not None]
            self._parent_step()
            if clamp is not None:
                for p in stepped:
                    p.clamp_(clamp[0], clamp[1])
            return loss
        stepped, sets = found
        written = []
        try:
            for group, count, params in sets:
                self._begin(group, count, params)
                try:
                    with torch.cuda.device(params[0].device):
                        ops.optim_step(self._kind, params, [p.grad for p in params],
                                       *([self.state[p][key] for p in params] for key in self._states(group)),
                                       clamp=clamp, **self._hyper(group, count))
                except BaseException:
                    self._abort(group, count, params)
                    raise
                self._advance(group, count, params)
                written += params
        finally:
            if written:      # also when a later set raised: what was launched was written
                torch.autograd.graph.increment_version(written)
        return loss


class Adam(_DeviceStep, torch.optim.Adam):
    _kind = "adam"

    def _states(self, group):
        return ("exp_avg", "exp_avg_sq")

    def _hyper(self, group, count):
        return dict(lr=group["lr"], betas=group["betas"], eps=group["eps"], weight_decay=group["weight_decay"], step=count)


class Adamax(_DeviceStep, torch.optim.Adamax):
    _kind = "adamax"

    def _states(self, group):
        return ("exp_avg", "exp_inf")

    def _hyper(self, group, count):
        return dict(lr=group["lr"], betas=group["betas"], eps=group["eps"], weight_decay=group["weight_decay"], step=count)


class RMSprop(_DeviceStep, torch.optim.RMSprop):
    _kind = "rmsprop"

    def _states(self, group):
        return ("square_avg",)

    def _hyper(self, group, count):
        return dict(lr=group["lr"], alpha=group["alpha"], eps=group["eps"], weight_decay=group["weight_decay"])


class SGD(_DeviceStep, torch.optim.SGD):
    """torch's SGD keeps no step count: a parameter's first step with momentum is the one that finds no `momentum_buffer`
    (buf = g), so the sets of a group are "first step" and "later step".  Without momentum there is no state at all."""
    _kind = "sgd"

    def _states(self, group):
        return ("momentum_buffer",) if group["momentum"] != 0 else ()

    def _init_state(self, group, state, p):
        pass

    def _count(self, group, state):
        return group["momentum"] != 0 and state.get("momentum_buffer") is None

    def _begin(self, group, first, params):
        if first:      # the kernel writes buf = g into them
            for p in params:
                self.state[p]["momentum_buffer"] = torch.empty_like(p, memory_format=torch.preserve_format)

    def _abort(self, group, first, params):
        if first:      # never written: the next step is still the first
            for p in params:
                self.state[p].pop("momentum_buffer", None)

    def _advance(self, group, count, params):
        pass

    def _hyper(self, group, first):
        return dict(lr=group["lr"], weight_decay=group["weight_decay"], momentum=group["momentum"],
                    dampening=group["dampening"], nesterov=group["nesterov"], first_step=first)
