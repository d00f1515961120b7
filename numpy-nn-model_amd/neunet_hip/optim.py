"""Fused optimizers -- drop-ins for CUDAFusedAdamW (experimental/optim/fused_adamw/fused_adamw.py:45-113)
and CUDAFusedMultiTensorAdamW (.../fused_adamw_multitensor.py:47-148), plus `Adam` / `AdamW` names that
select the L2-on-gradient (neunet/optim.py:17-33) or decoupled (optim.py:52-69) decay mode of the same
fused kernel, and the reference's seven other optimizers (optim.py:76-244: SGD, Momentum, RMSprop, Adagrad,
Adadelta, Adamax, NAdam) on the one-launch multi-tensor kernel of csrc/optim_rules.hip."""
import ctypes
import weakref
from ctypes import c_int64, c_void_p

from ._lib import call_hip_function, get_current_stream_ptr, load_hip_function
from .autograd import bump_param_epoch

DECOUPLED, L2_ON_GRAD = 0, 1


def _check_params(params, name="Fused AdamW"):
    import torch
    for p in params:
        if p.device != "cuda":
            raise ValueError(f"{name} only supports parameters on the HIP device ('cuda').")
        if p.data.dtype != torch.float32:
            raise ValueError(f"{name} only supports float32 parameters, got {p.data.dtype}")


class HIPFusedAdamW:
    """One launch per tensor (fused_adamw.py:64-109)."""
    decay_mode = DECOUPLED

    def __init__(self, params, lr: float = 0.01, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.01):
        import torch
        self.params = list(params)
        self.lr, self.betas, self.eps, self.weight_decay = lr, betas, eps, weight_decay
        _check_params(self.params)
        self.m = [torch.zeros_like(p.data) for p in self.params]
        self.v = [torch.zeros_like(p.data) for p in self.params]
        self.t = 0
        self.grad_scale = 1.0

    def step(self):
        self.t += 1
        bump_param_epoch()        # parameters change in place: deferred Linear outputs of this step are now stale
        stream = get_current_stream_ptr()
        for i, p in enumerate(self.params):
            if p.grad is None:
                continue
            g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
            if not p.data.is_contiguous():
                p.data = p.data.contiguous()
            call_hip_function("nnhipFusedAdamWStep", p.data, g, self.m[i], self.v[i], self.lr, self.betas[0],
                              self.betas[1], self.eps, self.weight_decay, self.t, p.data.numel(),
                              self.decay_mode, self.grad_scale, stream)

    def zero_grad(self):
        for p in self.params:
            p.grad = None


NORM_L2, NORM_INF = 0, 1                  # include/neunet_hip.h: NNHIP_NORM_*


def norm_type_id(norm_type):
    """2 / inf -> NNHIP_NORM_L2 / NNHIP_NORM_INF; anything else is a ValueError (no other p-norm has a kernel)."""
    try:
        v = float(norm_type)
    except (TypeError, ValueError):
        raise ValueError(f"norm_type must be 2.0 or float('inf'), got {norm_type!r}") from None
    if v == 2.0:
        return NORM_L2
    if v == float("inf"):
        return NORM_INF
    raise ValueError(f"norm_type must be 2.0 or float('inf'), got {norm_type!r}")


def check_max_norm(max_norm):
    """max_norm as a float; NaN, zero and negative values are a ValueError (the C entry answers NNHIP_EINVAL for them)."""
    try:
        v = float(max_norm)
    except (TypeError, ValueError):
        raise ValueError(f"max_norm must be a positive number, got {max_norm!r}") from None
    if not v > 0.0:
        raise ValueError(f"max_norm must be a positive number, got {max_norm!r}")
    return v


class _GradClipping:
    """Gradient clipping by global norm inside step(), shared by every multi-tensor optimizer here (extension: the reference has
    none).  `opt.max_grad_norm = 1.0` arms it: step() then launches nnhipGradNormMultiTensor on the tables it builds anyway --
    ONE launch that leaves norm, divisor and a non-finite flag in four device floats -- and binds the handle's gradient divisor
    to the divisor word, so the unchanged update launch applies torch's clip_coef without a pass over the gradients, a host read
    or a memset: legal in a captured step.  The norm is that of the EFFECTIVE gradient (grad_scale and the user's grad_divisor
    applied).  `opt.grad_norm_type` is 2.0 (default) or float('inf').  `opt.max_grad_norm = None` (default) disarms: step()
    makes exactly the calls it made before.  Arm before a GraphedTrainStep is built; a new max_grad_norm between replays takes
    effect at the next replay, as a new lr does.

    `last_grad_norm` / `last_grad_nonfinite`: 1-element device views of the words; reading them is the caller's
    synchronisation."""
    _max_grad_norm = None
    _grad_norm_type = 2.0
    _clip_words = None            # torch.zeros(4): norm, divisor, non-finite flag, max_norm for device-driven stepping
    _clip_divisor = None          # the view of word 1 the handle's divisor is bound to (one object: step() compares identities)
    _dev_max_norm = None          # the max_norm last written to word 3

    @property
    def max_grad_norm(self):
        return self._max_grad_norm

    @max_grad_norm.setter
    def max_grad_norm(self, value):
        self._max_grad_norm = None if value is None else check_max_norm(value)

    @property
    def grad_norm_type(self):
        return self._grad_norm_type

    @grad_norm_type.setter
    def grad_norm_type(self, value):
        norm_type_id(value)
        self._grad_norm_type = float(value)

    @property
    def last_grad_norm(self):
        return None if self._clip_words is None else self._clip_words[0:1]

    @property
    def last_grad_nonfinite(self):
        return None if self._clip_words is None else self._clip_words[2:3]

    def _sync_clip_words(self):
        """Word 3 follows max_grad_norm (a stream-ordered fill, only when it changed): what a captured norm launch reads."""
        if self._max_grad_norm is None:
            return
        if self._clip_words is None:
            import torch
            self._clip_words = torch.zeros(4, dtype=torch.float32, device="cuda")
            self._clip_divisor = self._clip_words[1:2]
            self._dev_max_norm = None
        if self._dev_max_norm != self._max_grad_norm:
            self._clip_words[3:4].fill_(self._max_grad_norm)
            self._dev_max_norm = self._max_grad_norm

    def _clip_launch(self, n, stream):
        """The norm launch over the first `n` entries of c_grads / c_sizes; returns the divisor word for the update to bind."""
        self._sync_clip_words()
        call_hip_function("nnhipGradNormMultiTensor", self.opt_ptr, n, ctypes.cast(self.c_grads, ctypes.POINTER(c_void_p)),
                          ctypes.cast(self.c_sizes, ctypes.POINTER(c_int64)), norm_type_id(self._grad_norm_type),
                          self._max_grad_norm, self.grad_divisor, 0 if self.device_step else self.t, self.grad_scale,
                          self._clip_words, stream)
        return self._clip_divisor


class HIPFusedMultiTensorAdamW(_GradClipping):
    """One launch for all tensors (fused_adamw_multitensor.py:88-144).  Pointer tables are ctypes arrays in
    host memory whose entries are device pointers -- same contract as the reference."""
    decay_mode = DECOUPLED

    def __init__(self, params, lr: float = 0.01, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.01):
        import torch
        self.params = list(params)
        self.lr, self.betas, self.eps, self.weight_decay = lr, betas, eps, weight_decay
        self.t = 0
        self.grad_scale = 1.0
        _check_params(self.params)
        self.m = [torch.zeros_like(p.data) for p in self.params]
        self.v = [torch.zeros_like(p.data) for p in self.params]
        self.device_step = False      # True: step count, lr, weight_decay, grad_scale live on the device (hipGraph replay)
        self._dev_hyper = None        # (lr, weight_decay, grad_scale) last written to the device state
        self.grad_divisor = None      # device float tensor (1 element): gradients are divided by it inside the kernel
        self._bound_divisor = None
        self.opt_ptr = load_hip_function("nnhipCreateFusedOptimizer")()
        if not self.opt_ptr:
            raise RuntimeError("nnhipCreateFusedOptimizer failed")
        n = len(self.params)
        self.c_params = (c_void_p * n)()
        self.c_grads = (c_void_p * n)()
        self.c_exp_avgs = (c_void_p * n)()
        self.c_exp_avg_sqs = (c_void_p * n)()
        self.c_sizes = (c_int64 * n)()
        self._in_backward = False     # fuse_backward(): the layers' backward kernels apply the update themselves when they can
        self._stepped_in_backward = False
        # the parameters know their optimizer (weakly): a backward kernel that produces ALL of its gradients may wait for
        # step() and take the update into its own launch (experimental/linear.py: _PendingMLPBackward) -- the default path
        self._ref = weakref.ref(self)
        self._index = {id(p): i for i, p in enumerate(self.params)}
        for p in self.params:
            p._opt_ref = self._ref

    def fuse_backward(self, enable: bool = True):
        """"Optimizer in backward" (extension; single process only): a backward kernel that produces ALL of this optimizer's
        gradients may apply the Adam update in its own epilogue -- today the README quick-start MLP's one-launch backward
        (experimental/linear.py: _mlp_chain_backward -> nnhipLinearReLULinearBackwardAdam).  step() then launches nothing for
        that iteration.  Same arithmetic, same results; call step() after every backward() (no gradient accumulation across
        backward passes, no all-reduce between them -- a GradBucket with hooks keeps the ordinary path)."""
        self._in_backward = bool(enable)
        for i, p in enumerate(self.params):
            if enable:
                p._fused_opt = (self, i)
            elif hasattr(p, "_fused_opt"):
                del p._fused_opt

    def can_fuse_into_backward(self):
        """Nothing stands between this optimizer's gradients and its update: no gradient divisor (clipping), no armed
        max_grad_norm (the norm needs every gradient before any update), no live collectives (data parallel: the gradients
        have to meet the other ranks' first)."""
        if self.grad_divisor is not None or self._max_grad_norm is not None:
            return False
        from .distributed import collectives_live
        return not collectives_live()

    def _update_table(self, params, step):
        """(optimizer handle, pointer table {p, m, v} x params, hyper-parameters, step) for a backward kernel that applies the
        update itself; None when `params` are not exactly this optimizer's parameters or one of them is not contiguous."""
        if len(params) != len(self.params) or len({id(p) for p in params}) != len(params):
            return None
        table = (c_void_p * (3 * len(params)))()
        for k, p in enumerate(params):
            i = self._index.get(id(p))
            if i is None or self.params[i] is not p or not p.data.is_contiguous():
                return None
            table[3 * k], table[3 * k + 1], table[3 * k + 2] = p.data.data_ptr(), self.m[i].data_ptr(), self.v[i].data_ptr()
        # the fused kernel reads the divisor from the library handle: a divisor bound by an earlier ordinary step() (clipping
        # switched on for a few steps, then back to None) must be unbound first -- it may point at freed memory by now
        if self._bound_divisor is not None:
            call_hip_function("nnhipFusedOptimizerSetGradDivisor", self.opt_ptr, None)
            self._bound_divisor = None
        if self.device_step:
            self.sync_device_hyper()
        return (self.opt_ptr, table, self.lr, self.betas[0], self.betas[1], self.eps, self.weight_decay,
                0 if self.device_step else step, self.decay_mode, self.grad_scale)

    def backward_update_args(self, params):
        """fuse_backward(True): for a backward kernel launched INSIDE backward() (step() has not been called yet: step t + 1)."""
        if not self._in_backward or self._stepped_in_backward or not self.can_fuse_into_backward():
            return None
        if any(getattr(p, "_fused_opt", (None,))[0] is not self for p in params):
            return None
        return self._update_table(params, self.t + 1)

    def pending_update_args(self, params, step):
        """For a backward launch that waited for the optimizer (the default path); `step` = the step number being applied."""
        if not self.can_fuse_into_backward():
            return None
        return self._update_table(params, step)

    def take_pending_backward(self):
        """A backward launch that is still waiting for this optimizer (experimental/linear.py: _PendingMLPBackward): launch it
        NOW with the update inside and let the coming step() only count.  For callers that look at the gradients between
        backward() and step() without changing them (GraphedTrainStep binds them to its bucket) -- without this their first
        look would run the plain backward and step() its own launch.  Returns True when the update has been applied."""
        pend = self.params[0]._pending if self.params else None
        if pend is None or self._stepped_in_backward or not pend.run_with_update(self, self.t + 1):
            return False
        self._stepped_in_backward = True
        bump_param_epoch()
        return True

    def __del__(self):
        ptr = getattr(self, "opt_ptr", None)
        if ptr:
            try:
                load_hip_function("nnhipDestroyFusedOptimizer")(ptr)
            except Exception:
                pass
            self.opt_ptr = None

    def step(self):
        self.t += 1
        bump_param_epoch()        # parameters change in place: deferred Linear outputs of this step are now stale
        if self._stepped_in_backward:          # a fused backward kernel already applied this step's update (fuse_backward)
            self._stepped_in_backward = False
            return
        pend = self.params[0]._pending if self.params else None
        if pend is not None:
            try:
                took = pend.run_with_update(self, self.t)
            except Exception:
                self.t -= 1                    # nothing was applied: the bias correction must not run one step ahead
                raise
            if took:
                return                         # the waiting backward launch took the update with it (one kernel, same values)
        idx = 0
        keep = []        # contiguous copies of strided gradients must outlive the single launch below: a freed block
        #                  could be handed to the next .contiguous() and two table entries would alias one buffer
        for i, p in enumerate(self.params):
            if p.grad is None:  # fused_adamw_multitensor.py:92-96: skip params without a gradient
                continue
            g = p.grad
            if not g.is_contiguous():
                g = g.contiguous()
                keep.append(g)
            if not p.data.is_contiguous():
                p.data = p.data.contiguous()
            self.c_params[idx] = p.data.data_ptr()
            self.c_grads[idx] = g.data_ptr()
            self.c_exp_avgs[idx] = self.m[i].data_ptr()
            self.c_exp_avg_sqs[idx] = self.v[i].data_ptr()
            self.c_sizes[idx] = p.data.numel()
            idx += 1
        if idx == 0:
            return
        div = self.grad_divisor
        if self._max_grad_norm is not None:    # armed: the norm launch first; the update divides by the word it leaves
            if self.device_step:
                self.sync_device_hyper()
            div = self._clip_launch(idx, get_current_stream_ptr())
        if div is not self._bound_divisor:
            call_hip_function("nnhipFusedOptimizerSetGradDivisor", self.opt_ptr, div)
            self._bound_divisor = div
        if self.device_step:
            self.sync_device_hyper()
        call_hip_function("nnhipFusedAdamWMultiTensorStep", self.opt_ptr, idx,
                          ctypes.cast(self.c_params, ctypes.POINTER(c_void_p)),
                          ctypes.cast(self.c_grads, ctypes.POINTER(c_void_p)),
                          ctypes.cast(self.c_exp_avgs, ctypes.POINTER(c_void_p)),
                          ctypes.cast(self.c_exp_avg_sqs, ctypes.POINTER(c_void_p)),
                          ctypes.cast(self.c_sizes, ctypes.POINTER(c_int64)),
                          self.lr, self.betas[0], self.betas[1], self.eps, self.weight_decay,
                          0 if self.device_step else self.t, self.decay_mode, self.grad_scale,
                          get_current_stream_ptr())

    def use_device_step(self, enable: bool = True):
        """Move the step counter AND lr / weight_decay / grad_scale to device memory (needed before capturing step()
        into a hipGraph: host values would be frozen into the captured kernel arguments).  While enabled, assign
        `opt.lr`, `opt.weight_decay`, `opt.grad_scale` as usual: `sync_device_hyper()` (called by step() and by
        GraphedTrainStep before every replay) writes changed values to the device with one tiny stream-ordered launch."""
        if enable:
            call_hip_function("nnhipFusedOptimizerSetStep", self.opt_ptr, self.t, get_current_stream_ptr())
            self._dev_hyper = None
            self.device_step = True
            self.sync_device_hyper()
        else:
            self.device_step = False

    def sync_device_hyper(self):
        cur = (float(self.lr), float(self.weight_decay), float(self.grad_scale))
        if self.device_step and cur != self._dev_hyper:
            call_hip_function("nnhipFusedOptimizerSetHyper", self.opt_ptr, cur[0], cur[1], cur[2], get_current_stream_ptr())
            self._dev_hyper = cur
        if self.device_step:
            self._sync_clip_words()           # a changed max_grad_norm -> word 3, which a captured norm launch reads

    def zero_grad(self):
        for p in self.params:
            p.grad = None


class AdamW(HIPFusedMultiTensorAdamW):
    """neunet.optim.AdamW (optim.py:39-73) on the fused multi-tensor kernel."""


class Adam(HIPFusedMultiTensorAdamW):
    """neunet.optim.Adam (optim.py:4-37): weight decay is L2-on-gradient; default weight_decay=0."""
    decay_mode = L2_ON_GRAD

    def __init__(self, params, lr: float = 0.01, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0):
        super().__init__(params, lr, betas, eps, weight_decay)


# ------------------------------------------------------------------ SGD, Momentum, RMSprop, Adagrad, Adadelta, Adamax, NAdam
# include/neunet_hip.h: NNHIP_OPT_*
RULE_SGD, RULE_MOMENTUM, RULE_RMSPROP, RULE_ADAGRAD, RULE_ADADELTA, RULE_ADAMAX, RULE_NADAM = range(7)


class _RuleOptimizer(_GradClipping):
    """What the seven optimizers below share: one launch for all tensors (nnhipOptimizerRuleMultiTensorStep) on a handle of
    nnhipCreateFusedOptimizer, with everything of HIPFusedMultiTensorAdamW that is not Adam's -- `grad_scale`, `grad_divisor`,
    `max_grad_norm` / `grad_norm_type` (_GradClipping),
    `use_device_step` / `sync_device_hyper` (hipGraph replay: GraphedTrainStep takes these classes as it takes Adam),
    parameters without a gradient skipped, strided gradients copied.  A subclass names its rule, its state streams (`m`, `v`:
    the reference's attribute names) and its two coefficients.

    Never part of the optimizer-in-backward path: the README MLP's deferred backward launch applies ADAM in its epilogue, so these
    classes do not register themselves with their parameters (`_opt_ref`), have no fuse_backward(), and answer
    can_fuse_into_backward() False / pending_update_args() None; step() reads every gradient, which runs a still-pending
    backward launch plain.

    `t` counts step() calls in every class (the reference keeps it only where the rule has a bias correction)."""
    rule = None
    n_state = 0
    _stepped_in_backward = False      # no backward kernel ever applies these rules

    def _setup(self, params, lr):
        import torch
        self.params = list(params)
        self.lr = lr
        _check_params(self.params, type(self).__name__)
        if self.n_state >= 1:
            self.m = [torch.zeros_like(p.data) for p in self.params]
        if self.n_state >= 2:
            self.v = [torch.zeros_like(p.data) for p in self.params]
        self.t = 0
        self.grad_scale = 1.0
        self.device_step = False      # True: step count, lr, grad_scale live on the device (hipGraph replay)
        self._dev_hyper = None        # (lr, grad_scale) last written to the device state
        self.grad_divisor = None      # device float tensor (1 element): gradients are divided by it inside the kernel
        self._bound_divisor = None
        self.opt_ptr = load_hip_function("nnhipCreateFusedOptimizer")()
        if not self.opt_ptr:
            raise RuntimeError("nnhipCreateFusedOptimizer failed")
        n = len(self.params)
        self.c_params = (c_void_p * n)()
        self.c_grads = (c_void_p * n)()
        self.c_state1 = (c_void_p * n)()
        self.c_state2 = (c_void_p * n)()
        self.c_sizes = (c_int64 * n)()

    def _coefficients(self):
        """(coef1, coef2, eps) of nnhipOptimizerRuleMultiTensorStep."""
        return 0.0, 0.0, 0.0

    def can_fuse_into_backward(self):
        return False

    def pending_update_args(self, params, step):
        return None

    def __del__(self):
        ptr = getattr(self, "opt_ptr", None)
        if ptr:
            try:
                load_hip_function("nnhipDestroyFusedOptimizer")(ptr)
            except Exception:
                pass
            self.opt_ptr = None

    def step(self):
        self.t += 1
        bump_param_epoch()        # parameters change in place: deferred Linear outputs of this step are now stale
        idx = 0
        keep = []        # contiguous copies of strided gradients must outlive the single launch below
        for i, p in enumerate(self.params):
            g = p.grad            # a backward launch still waiting for an Adam step() runs now, without an update
            if g is None:
                continue
            if not g.is_contiguous():
                g = g.contiguous()
                keep.append(g)
            if not p.data.is_contiguous():
                p.data = p.data.contiguous()
            self.c_params[idx] = p.data.data_ptr()
            self.c_grads[idx] = g.data_ptr()
            if self.n_state >= 1:
                self.c_state1[idx] = self.m[i].data_ptr()
            if self.n_state >= 2:
                self.c_state2[idx] = self.v[i].data_ptr()
            self.c_sizes[idx] = p.data.numel()
            idx += 1
        if idx == 0:
            return
        div = self.grad_divisor
        if self._max_grad_norm is not None:    # armed: the norm launch first; the update divides by the word it leaves
            if self.device_step:
                self.sync_device_hyper()
            div = self._clip_launch(idx, get_current_stream_ptr())
        if div is not self._bound_divisor:
            call_hip_function("nnhipFusedOptimizerSetGradDivisor", self.opt_ptr, div)
            self._bound_divisor = div
        if self.device_step:
            self.sync_device_hyper()
        c1, c2, eps = self._coefficients()
        call_hip_function("nnhipOptimizerRuleMultiTensorStep", self.opt_ptr, self.rule, idx,
                          ctypes.cast(self.c_params, ctypes.POINTER(c_void_p)),
                          ctypes.cast(self.c_grads, ctypes.POINTER(c_void_p)),
                          ctypes.cast(self.c_state1, ctypes.POINTER(c_void_p)) if self.n_state >= 1 else None,
                          ctypes.cast(self.c_state2, ctypes.POINTER(c_void_p)) if self.n_state >= 2 else None,
                          ctypes.cast(self.c_sizes, ctypes.POINTER(c_int64)),
                          self.lr, c1, c2, eps, 0 if self.device_step else self.t, self.grad_scale,
                          get_current_stream_ptr())

    def use_device_step(self, enable: bool = True):
        """Move the step counter AND lr / grad_scale to device memory (needed before capturing step() into a hipGraph: host
        values would be frozen into the captured kernel arguments).  While enabled, assign `opt.lr` and `opt.grad_scale` as
        usual: `sync_device_hyper()` (called by step() and by GraphedTrainStep before every replay) writes changed values to the
        device with one tiny stream-ordered launch.  The rule's coefficients and eps stay launch arguments."""
        if enable:
            call_hip_function("nnhipFusedOptimizerSetStep", self.opt_ptr, self.t, get_current_stream_ptr())
            self._dev_hyper = None
            self.device_step = True
            self.sync_device_hyper()
        else:
            self.device_step = False

    def sync_device_hyper(self):
        cur = (float(self.lr), float(self.grad_scale))
        if self.device_step and cur != self._dev_hyper:
            call_hip_function("nnhipFusedOptimizerSetHyper", self.opt_ptr, cur[0], 0.0, cur[1], get_current_stream_ptr())
            self._dev_hyper = cur
        if self.device_step:
            self._sync_clip_words()           # a changed max_grad_norm -> word 3, which a captured norm launch reads

    def zero_grad(self):
        for p in self.params:
            p.grad = None


class SGD(_RuleOptimizer):
    """neunet.optim.SGD (optim.py:76-90): p -= lr * g.  No state."""
    rule, n_state = RULE_SGD, 0

    def __init__(self, params, lr: float = 0.01):
        self._setup(params, lr)


class Momentum(_RuleOptimizer):
    """neunet.optim.Momentum (optim.py:92-110): m = momentum * m + (1 - momentum) * g; p -= m * lr.
    zero_grad() sets the gradients to None like every optimizer here; the reference's Momentum.zero_grad zero-fills existing
    gradients instead (optim.py:108-110) -- the next backward pass overwrites either."""
    rule, n_state = RULE_MOMENTUM, 1

    def __init__(self, params, lr=0.01, momentum: float = 0.9):
        self.momentum = momentum
        self._setup(params, lr)

    def _coefficients(self):
        return self.momentum, 0.0, 0.0


class RMSprop(_RuleOptimizer):
    """neunet.optim.RMSprop (optim.py:113-132): m = alpha * m + (1 - alpha) * g^2; p -= lr * g / (sqrt(m) + eps)."""
    rule, n_state = RULE_RMSPROP, 1

    def __init__(self, params, lr: float = 0.01, alpha: float = 0.99, eps: float = 1e-8):
        self.alpha, self.eps = alpha, eps
        self._setup(params, lr)

    def _coefficients(self):
        return self.alpha, 0.0, self.eps


class Adagrad(_RuleOptimizer):
    """neunet.optim.Adagrad (optim.py:135-153): m += g^2; p -= lr * g / (sqrt(m) + eps)."""
    rule, n_state = RULE_ADAGRAD, 1

    def __init__(self, params, lr: float = 0.01, eps: float = 1e-8):
        self.eps = eps
        self._setup(params, lr)

    def _coefficients(self):
        return 0.0, 0.0, self.eps


class Adadelta(_RuleOptimizer):
    """neunet.optim.Adadelta (optim.py:156-181): m = rho * m + (1 - rho) * g^2; dx = -sqrt(v + eps) / sqrt(m + eps) * g;
    v = rho * v + (1 - rho) * dx^2; p += dx.  `lr` is accepted and IGNORED: the reference stores it and never uses it."""
    rule, n_state = RULE_ADADELTA, 2

    def __init__(self, params, lr: float = 1.0, rho: float = 0.9, eps: float = 1e-6):
        self.rho, self.eps = rho, eps
        self._setup(params, lr)

    def _coefficients(self):
        return self.rho, 0.0, self.eps


class Adamax(_RuleOptimizer):
    """neunet.optim.Adamax (optim.py:184-211): m as Adam; v = max(beta2 * v, |g|); p -= lr * (m / (1 - beta1^t)) / (v + eps)."""
    rule, n_state = RULE_ADAMAX, 2

    def __init__(self, params, lr: float = 0.002, betas=(0.9, 0.999), eps: float = 1e-8):
        self.betas, self.eps = betas, eps
        self._setup(params, lr)

    def _coefficients(self):
        return self.betas[0], self.betas[1], self.eps


class NAdam(_RuleOptimizer):
    """neunet.optim.NAdam (optim.py:214-244): m, v as Adam; m_hat = m / bc1 + (1 - beta1) * g / bc1;
    p -= lr * m_hat / (sqrt(v / bc2) + eps), bc = 1 - beta^t."""
    rule, n_state = RULE_NADAM, 2

    def __init__(self, params, lr: float = 0.002, betas=(0.9, 0.999), eps: float = 1e-8):
        self.betas, self.eps = betas, eps
        self._setup(params, lr)

    def _coefficients(self):
        return self.betas[0], self.betas[1], self.eps


CUDAFusedAdamW, CUDAFusedMultiTensorAdamW = HIPFusedAdamW, HIPFusedMultiTensorAdamW
