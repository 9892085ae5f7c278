"""`optimizer.step()` on the device: Adam, SGD and RMSprop as the reference's `utils.create_optimizer` builds them
(utils/utils.py:61-79), every served tensor of a step in ONE launch of csrc/optimizer.hip (tpnet_optim_step) per
`tpnet_optim_max_tensors()` tensors.

`DeviceAdam`, `DeviceSGD` and `DeviceRMSprop` are `torch.optim.Optimizer` subclasses with the `param_groups` keys, the state keys and the
state tensors of `torch.optim.Adam` / `SGD` / `RMSprop`: a `state_dict()` of either side loads into the other.  What the kernel does not
serve -- amsgrad, maximize, momentum, centered, decoupled decay, capturable, differentiable -- is a ValueError, in the constructor and,
for options that arrive through `load_state_dict` or an edited param group, in `step()`.

Which tensors the kernel serves is decided in every `step()` (the reference builds its optimizer before it moves the model,
train_link_prediction.py:220-223): a Parameter and its gradient on one GPU, both fp32, contiguous and dense.  Any other tensor takes
torch's own single-tensor functional update (`foreach=False`) on the same state tensors in the same call; that is logged once per
optimizer.  A Parameter without a gradient is skipped and its `step` does not advance.

The version contract: the fused forwards cache their split-bf16 weight images under `(data_ptr, _version)` of the Parameters
(`_dense.param_key`).  The kernel writes through raw pointers, so `step()` ends with `torch.autograd.graph.increment_version` on the
Parameters it served -- without it every cached image would keep serving the weights from before the step.

`step()` does not synchronise: the table of pointers travels by value in the kernel's arguments, `state['step']` stays a CPU scalar
as torch keeps it (the served tensors' scalars are views into one CPU buffer, so that all of them advance in one host op; a `step`
tensor that `load_state_dict` brought is read once, then counted on the host), and the bias corrections are formed on the host in
double, as torch forms them.

`optimizer_step_host` restates the kernel's rule in numpy, fp32, in the kernel's operation order: the reference of the CPU tests and,
bit for bit, of the GPU tests."""
import logging
import struct

import numpy as np
import torch
from torch.optim.adam import adam as _torch_adam
from torch.optim.rmsprop import rmsprop as _torch_rmsprop
from torch.optim.sgd import sgd as _torch_sgd

from . import _lib
from ._lib import OPTIM_ADAM, OPTIM_RMSPROP, OPTIM_SGD

log = logging.getLogger(__name__)

RULES = {"Adam": OPTIM_ADAM, "SGD": OPTIM_SGD, "RMSprop": OPTIM_RMSPROP}
_ENTRY = struct.Struct("=4Qq8fII")                  # tpnet_optim_tensor: p, g, s1, s2, n, c[8], flags, reserved
_F32 = struct.Struct("=8f")


def adam_scalars(lr, beta1, beta2, eps, weight_decay, step):
    """c[8] of an Adam entry at step `step` (1, 2, ...): python floats, formed in double as torch's single-tensor Adam forms them; the
    entry's store rounds each once to fp32."""
    return (lr / (1.0 - beta1 ** step), weight_decay, beta1, 1.0 - beta1, beta2, 1.0 - beta2, (1.0 - beta2 ** step) ** 0.5, eps)


def sgd_scalars(lr, weight_decay):
    return (lr, weight_decay, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)


def rmsprop_scalars(lr, alpha, eps, weight_decay):
    return (lr, weight_decay, alpha, 1.0 - alpha, eps, 0.0, 0.0, 0.0)


def optimizer_step_host(rule, p, g, s1, s2, scalars):
    """The kernel's rule on numpy arrays: -> (p', s1', s2') fp32 (s1' / s2' None where the rule has no such state).  rule: 'Adam', 'SGD',
    'RMSprop' or its code; scalars: the entry's c[8] (each is rounded once to fp32 here, as the entry's store rounds it).  Every line
    is one fp32 operation of csrc/optimizer.hip: optim_elem, in its order."""
    rule = RULES.get(rule, rule)
    c = np.array(_F32.unpack(_F32.pack(*scalars)), dtype=np.float32)
    p, g = np.asarray(p, dtype=np.float32), np.asarray(g, dtype=np.float32)
    with np.errstate(all="ignore"):
        if c[1] != 0:
            t = c[1] * p
            g = g + t
        if rule == OPTIM_ADAM:
            a = c[2] * np.asarray(s1, dtype=np.float32)
            b = c[3] * g
            m = a + b
            d = c[4] * np.asarray(s2, dtype=np.float32)
            e = c[5] * g
            e = e * g
            v = d + e
            den = np.sqrt(v)
            den = den / c[6]
            den = den + c[7]
            q = m / den
            u = c[0] * q
            return p - u, m, v
        if rule == OPTIM_SGD:
            u = c[0] * g
            return p - u, None, None
        if rule == OPTIM_RMSPROP:
            a = c[2] * np.asarray(s1, dtype=np.float32)
            e = c[3] * g
            e = e * g
            s = a + e
            den = np.sqrt(s)
            den = den + c[4]
            q = g / den
            u = c[0] * q
            return p - u, s, None
    raise ValueError(f"optimizer_step_host: unknown rule {rule!r}")


def _served(p, g):
    """torch lets a gradient differ from its Parameter in strides and layout only (dtype, device and shape are checked when it is set)."""
    return (p.is_cuda and p.dtype is torch.float32 and g.dtype is torch.float32 and p.layout is torch.strided
            and g.layout is torch.strided and g.is_cuda and p.is_contiguous() and g.is_contiguous())


def _state_served(p, s):
    return s.device == p.device and s.dtype is torch.float32 and s.is_contiguous() and s.numel() == p.numel()


class _DeviceOptimizer(torch.optim.Optimizer):
    """What the three classes share: the walk over the groups, the table, the launches, the version bump and the step counts.

    The step counts: torch keeps `state['step']` as one CPU scalar per tensor and adds 1 to each in every step, 38 small host ops.
    Here the scalars of the tensors the kernel serves are 0-dim views into ONE CPU buffer (`_steps`) -- to a reader the same fp32 CPU
    scalars -- so a step in which all of them advance is one `add_`, and the host keeps each count as an int beside it (`_slots`), so
    nothing is read back.  A `step` tensor that arrives from outside (load_state_dict, a state set by hand) is read once and moved
    into the buffer; a tensor that leaves for torch's update gets a scalar of its own again."""
    rule = None
    state_names = ()                    # the state tensors the kernel reads, in the entry's order (s1, s2)
    _unserved = ()                      # (param group key, the value the kernel serves)

    def __init__(self, params, defaults):
        super().__init__(params, defaults)
        self._reset_counts()
        self._logged = False
        for group in self.param_groups:
            self._check_group(group)

    def __setstate__(self, state):      # load_state_dict, unpickling, deepcopy: the state tensors are new objects
        super().__setstate__(state)
        self._reset_counts()
        self.__dict__.setdefault("_logged", False)

    def _reset_counts(self):
        self._steps = None              # CPU float32 [capacity]
        self._used = 0                  # slots handed out
        self._live = 0                  # slots whose view is some tensor's state['step']
        self._slots = {}                # id(Parameter) -> [view, count, the state tensors found fit for the kernel]

    def _check_group(self, group):
        for key, served in self._unserved:
            if group.get(key, served) != served:
                raise ValueError(f"{type(self).__name__}: {key}={group[key]!r} is not served by the device step (only {served!r})")
        for key in ("lr", "weight_decay", "eps", "alpha"):
            if key in group and not (isinstance(group[key], (int, float)) and group[key] >= 0.0):
                raise ValueError(f"{type(self).__name__}: invalid {key}: {group[key]!r}")
        if "betas" in group and not all(isinstance(b, (int, float)) and 0.0 <= b < 1.0 for b in group["betas"]):
            raise ValueError(f"{type(self).__name__}: invalid betas: {group['betas']!r}")

    def _new_state(self, p, state):
        state["step"] = torch.tensor(0.0, dtype=torch.float32)
        for name in self.state_names:
            state[name] = torch.zeros_like(p, memory_format=torch.preserve_format)

    def _slot(self, p, state):
        """The slot of a tensor on the kernel's route, or None where its state is not what the kernel reads."""
        slot = self._slots.get(id(p))
        step_t = state["step"]
        if slot is not None and slot[0] is step_t:
            for name, s in zip(self.state_names, slot[2]):
                if state[name] is not s:
                    break
            else:
                return slot
            slot[2] = ()
        states = tuple(state[name] for name in self.state_names)
        if step_t.is_cuda or not all(_state_served(p, s) for s in states):
            return None
        if slot is None or slot[0] is not step_t:
            if self._steps is None:
                self._steps = torch.zeros(sum(len(g["params"]) for g in self.param_groups) + 64, dtype=torch.float32)
            if self._used == self._steps.numel():                       # (tensors added later than the buffer was sized: their own scalar)
                slot = [step_t, int(step_t), states]
            else:
                if slot is not None and slot[0]._base is self._steps:
                    self._live -= 1
                count = int(step_t)
                view = self._steps[self._used]
                view.fill_(count)
                state["step"] = view
                self._used += 1
                self._live += 1
                slot = [view, count, states]
            self._slots[id(p)] = slot
        slot[2] = states
        return slot

    def _leave(self, p, state):
        """A tensor takes torch's update: its `step` is a scalar of its own, which torch's function advances."""
        slot = self._slots.pop(id(p), None)
        if slot is not None and slot[0]._base is self._steps and state["step"] is slot[0]:
            state["step"] = slot[0].clone()
            self._live -= 1

    def _scalars(self, group, t):
        raise NotImplementedError

    def _torch_update(self, p, g, group, state):
        raise NotImplementedError

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        stateful = self.rule != OPTIM_SGD             # (torch's SGD without momentum keeps no state entry at all)
        names = self.state_names
        tables = {}                                   # device index -> [bytearray of entries, the Parameters, the device]
        advanced = []                                 # slots that advance in this step
        n_other = 0
        pack = _ENTRY.pack
        for group in self.param_groups:
            self._check_group(group)
            memo = {}
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                state = slot = None
                if stateful:
                    state = self.state[p]
                    if len(state) == 0:
                        self._new_state(p, state)
                if _served(p, g) and (not stateful or (slot := self._slot(p, state)) is not None):
                    t = 0
                    if stateful:
                        t = slot[1] = slot[1] + 1
                        advanced.append(slot)
                    c = memo.get(t)
                    if c is None:
                        c = memo[t] = self._scalars(group, t)
                    tab = tables.get(p.get_device())
                    if tab is None:
                        tab = tables[p.get_device()] = [bytearray(), [], p.device]
                    tab[1].append(p)
                    n = p.numel()
                    if n:                                                # (an empty tensor may have no pointer to give)
                        tab[0] += pack(p.data_ptr(), g.data_ptr(), state[names[0]].data_ptr() if names else 0,
                                       state[names[1]].data_ptr() if len(names) > 1 else 0, n, *c, 0, 0)
                else:
                    if stateful:
                        self._leave(p, state)
                    self._torch_update(p, g, group, state)
                    n_other += 1
        if advanced:
            own = [s[0] for s in advanced if s[0]._base is not self._steps]
            if len(advanced) - len(own) == self._live:                   # every tensor of the buffer advances: one host op
                self._steps.add_(1)
            else:
                own = [s[0] for s in advanced]
            for step_t in own:
                step_t += 1
        if n_other and not self._logged:
            self._logged = True
            log.warning("%s: %d tensor(s) are not fp32, contiguous, dense and on a GPU with their gradients: they take torch's "
                        "single-tensor update in this and later steps (logged once)", type(self).__name__, n_other)
        if tables:
            lib = _lib.load()
            for buf, served, device in tables.values():
                raw = (_lib.C.c_char * len(buf)).from_buffer(buf)
                stream = torch.cuda.current_stream(device).cuda_stream
                if device.index != torch.cuda.current_device():
                    with torch.cuda.device(device):
                        rc = lib.tpnet_optim_step(self.rule, raw, len(buf) // _ENTRY.size, stream)
                else:
                    rc = lib.tpnet_optim_step(self.rule, raw, len(buf) // _ENTRY.size, stream)
                _lib.check(rc, "optim_step")
                torch.autograd.graph.increment_version(served)      # the kernel wrote through raw pointers: caches keyed by _version
        return loss


class DeviceAdam(_DeviceOptimizer):
    """torch.optim.Adam(params, lr, betas, eps, weight_decay) with the step on the device."""
    rule = OPTIM_ADAM
    state_names = ("exp_avg", "exp_avg_sq")
    _unserved = (("amsgrad", False), ("maximize", False), ("capturable", False), ("differentiable", False),
                 ("decoupled_weight_decay", False))

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None, maximize=False,
                 capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                                      foreach=foreach, capturable=capturable, differentiable=differentiable, fused=fused,
                                      decoupled_weight_decay=decoupled_weight_decay))

    def _scalars(self, group, t):
        b1, b2 = group["betas"]
        return adam_scalars(group["lr"], b1, b2, group["eps"], group["weight_decay"], t)

    def _torch_update(self, p, g, group, state):
        b1, b2 = group["betas"]
        _torch_adam([p], [g], [state["exp_avg"]], [state["exp_avg_sq"]], [], [state["step"]], foreach=False, capturable=False,
                    differentiable=False, fused=False, has_complex=torch.is_complex(p), decoupled_weight_decay=False, amsgrad=False,
                    beta1=b1, beta2=b2, lr=group["lr"], weight_decay=group["weight_decay"], eps=group["eps"], maximize=False)


class DeviceSGD(_DeviceOptimizer):
    """torch.optim.SGD(params, lr, weight_decay=...) -- momentum 0 -- with the step on the device."""
    rule = OPTIM_SGD
    _unserved = (("momentum", 0), ("dampening", 0), ("nesterov", False), ("maximize", False), ("differentiable", False))

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, maximize=False, foreach=None,
                 differentiable=False, fused=None):
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                                      maximize=maximize, foreach=foreach, differentiable=differentiable, fused=fused))

    def _scalars(self, group, t):
        return sgd_scalars(group["lr"], group["weight_decay"])

    def _torch_update(self, p, g, group, state):
        _torch_sgd([p], [g], [None], has_sparse_grad=g.is_sparse, foreach=False, fused=False, weight_decay=group["weight_decay"],
                   momentum=0, lr=group["lr"], dampening=0, nesterov=False, maximize=False)


class DeviceRMSprop(_DeviceOptimizer):
    """torch.optim.RMSprop(params, lr, alpha, eps, weight_decay) -- momentum 0, not centered -- with the step on the device."""
    rule = OPTIM_RMSPROP
    state_names = ("square_avg",)
    _unserved = (("momentum", 0), ("centered", False), ("maximize", False), ("capturable", False), ("differentiable", False))

    def __init__(self, params, lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0, momentum=0, centered=False, capturable=False,
                 foreach=None, maximize=False, differentiable=False):
        super().__init__(params, dict(lr=lr, momentum=momentum, alpha=alpha, eps=eps, centered=centered, weight_decay=weight_decay,
                                      capturable=capturable, foreach=foreach, maximize=maximize, differentiable=differentiable))

    def _scalars(self, group, t):                       # (the rule has no bias correction: one set of scalars per group)
        return rmsprop_scalars(group["lr"], group["alpha"], group["eps"], group["weight_decay"])

    def _torch_update(self, p, g, group, state):
        _torch_rmsprop([p], [g], [state["square_avg"]], [], [], [state["step"]], foreach=False, maximize=False, differentiable=False,
                       capturable=False, has_complex=torch.is_complex(p), lr=group["lr"], alpha=group["alpha"], eps=group["eps"],
                       weight_decay=group["weight_decay"], momentum=0, centered=False)
