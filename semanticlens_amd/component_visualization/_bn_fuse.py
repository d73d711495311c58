"""Run the probed model's inference BatchNorm2d on the library's K16 kernels while its hooks are registered.

``substitute(model)`` swaps instance ``forward`` attributes and returns the function that removes them again; nothing else of
the model is touched and outside the ``with`` block of :meth:`ActCache.hook_context` the model is exactly the user's.

* Every plain ``BatchNorm2d`` gets a ``forward`` that calls ``sl_batchnorm_infer`` when the call is eligible and the class's
  own ``forward`` otherwise.  The module is still *called*, so its hooks fire as before.
* Every module that directly owns a ``BatchNorm2d`` is traced with ``torch.fx`` — all of its children are leaves, so they are
  still called as modules and their hooks fire — and the patterns ``bn -> relu``, ``bn -> add(., other) -> relu`` and
  ``bn -> relu -> max_pool2d`` (the stem) are replaced by one fused call each.  A module that does not trace
  keeps its own ``forward``.
* Where the ``other`` of ``bn -> add(., other) -> relu`` is the output of a plain ``nn.Sequential`` that ends in a plain
  ``BatchNorm2d`` (the shortcut of a stage's first block) the owner gets a second graph: the Sequential's
  leading children are called where the Sequential was, each as a module, and the tail is one call that normalises both
  operands (``sl_batchnorm_infer_add_bn_relu``).  The owner runs that graph while nothing hooks the Sequential, its norm, the
  traced norm or the activation and the Sequential's children are the traced ones, and the first graph otherwise.

* Where the BatchNorm2d of ``bn -> add(., other) -> relu`` normalises the output of a plain pointwise ``nn.Conv2d`` of 64 -> 256
  channels (stride 1, no padding, dilation 1, one group, no bias: ``conv3`` of layer1's blocks) the owner gets a further graph
   in which convolution and tail are one call, ``sl_conv1x1_bn_add_relu``; where the shortcut is exactly
  ``Sequential(conv, bn)`` with such a convolution too, both products and the K19 tail are one call,
  ``sl_conv1x1_bn_add_conv1x1_bn_relu``.  A fused convolution is not *called* any more, so the owner runs this graph only while
  nothing hooks it (and the K16 / K19 conditions hold) and falls back one level, to the graphs above, otherwise.
  ``SEMANTICLENS_AMD_FUSE_CONV=0`` switches this level off.

Eligibility is decided per call (``_eligible``): eval mode with running statistics and affine parameters, fp32 on a HIP device,
NCHW-contiguous, grad mode off, MIOpen enabled, and for the fused patterns no hook on the norm or the activation, whose separate
outputs disappear.  The pooled form also needs pool parameters the kernel takes (read from the module at every call), no
``ceil_mode`` or ``return_indices`` and no hook on the pool; otherwise it falls back one level, to the fused ``bn -> relu`` and
the user's pool module.  Anything else runs the modules as the user wrote them.

Proof before trust: the first time a site runs an epilogue, the same input also goes through ``F.batch_norm`` (+ add, ``relu_``)
— the functional forms, so that no hook fires twice — and the bit patterns must be equal; otherwise the site is dropped with
one warning.  Verified sites are kept per model (weakly), so a second visualizer over the same model pays nothing.  For a
fused convolution the proof runs ``F.conv2d`` in front of those, and what it has proven is kept per input shape and
``torch.backends.cudnn`` flags: MIOpen chooses its solver, and with it the order of the sum over input channels, per shape.

``SEMANTICLENS_AMD_FUSE_BN=0`` switches all of this off.
"""
from __future__ import annotations

import inspect
import operator
import os
import warnings
import weakref

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _native as N

_BN_FORWARD = nn.modules.batchnorm._BatchNorm.forward
_PLANS: "weakref.WeakKeyDictionary[nn.Module, _Plan]" = weakref.WeakKeyDictionary()
_ADDS = (operator.add, operator.iadd, torch.add)
_RELUS = (F.relu, torch.relu, torch.relu_)
_POOL_ARGS = ("kernel_size", "stride", "padding", "dilation", "ceil_mode", "return_indices")  # F.max_pool2d's, after the input


def enabled() -> bool:
    return os.environ.get("SEMANTICLENS_AMD_FUSE_BN", "1") != "0"


def conv_enabled() -> bool:
    return enabled() and os.environ.get("SEMANTICLENS_AMD_FUSE_CONV", "1") != "0"


def _plain_bn(m) -> bool:
    return isinstance(m, nn.BatchNorm2d) and type(m).forward is _BN_FORWARD


def _plain_relu(m) -> bool:
    return isinstance(m, nn.ReLU) and type(m).forward is nn.ReLU.forward


def _plain_seq(m) -> bool:
    return isinstance(m, nn.Sequential) and type(m).forward is nn.Sequential.forward


def _plain_pool(m) -> bool:
    return isinstance(m, nn.MaxPool2d) and type(m).forward is nn.MaxPool2d.forward


def _tail_conv(m) -> bool:
    """A convolution the K27 kernels compute: plain, pointwise, 64 -> 256 channels, nothing else.  (Read from the module at every
    use: the user may have changed it since the trace.)"""
    return (isinstance(m, nn.Conv2d) and type(m).forward is nn.Conv2d.forward and m.in_channels == N.CONV_TAIL_IN
            and m.out_channels == N.CONV_TAIL_OUT and tuple(m.kernel_size) == (1, 1) and tuple(m.stride) == (1, 1)
            and m.padding in ((0, 0), 0) and tuple(m.dilation) == (1, 1) and m.groups == 1 and m.bias is None
            and m.padding_mode == "zeros")


def _pair(v):
    if isinstance(v, int) and not isinstance(v, bool):
        return (v, v)
    if isinstance(v, (tuple, list)) and len(v) == 2 and all(isinstance(e, int) and not isinstance(e, bool) for e in v):
        return tuple(v)
    return None


def _pool_params(kernel_size, stride=None, padding=0, dilation=1, ceil_mode=False, return_indices=False):
    """((kh, kw), (sh, sw), (ph, pw)) when the library's pooled epilogue computes this max_pool2d, else None."""
    if ceil_mode or return_indices or _pair(dilation) != (1, 1):
        return None
    k, p = _pair(kernel_size), _pair(padding)
    s = k if stride is None or stride == [] or stride == () else _pair(stride)
    if k is None or s is None or p is None or not N.bn_pool_supported(k, s, p):
        return None
    return k, s, p


def _hooked(m: nn.Module) -> bool:
    mod = nn.modules.module
    return bool(m._forward_hooks or m._forward_pre_hooks or mod._global_forward_hooks or mod._global_forward_pre_hooks)


def _streamable(t) -> bool:
    """A contiguous NCHW fp32 device tensor the kernels read or write with 16-byte accesses."""
    return (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype is torch.float32 and t.dim() == 4 and not t.requires_grad
            and t.is_contiguous() and not t.is_contiguous(memory_format=torch.channels_last) and t.data_ptr() % 16 == 0)


def _conv_operands(conv: nn.Conv2d, x) -> bool:
    """``x`` and ``conv.weight`` as the K27 kernels read them: fp32, contiguous, on one device."""
    w = conv.weight
    return (_streamable(x) and x.shape[1] == N.CONV_TAIL_IN and x.numel() > 0
            and x.numel() // N.CONV_TAIL_IN * N.CONV_TAIL_OUT <= N.CONV_TAIL_MAX_ELEMENTS and isinstance(w, torch.Tensor)
            and w.dtype is torch.float32 and w.device == x.device and w.is_contiguous() and w.data_ptr() % 16 == 0
            and tuple(w.shape) == (N.CONV_TAIL_OUT, N.CONV_TAIL_IN, 1, 1))


def _solver_key(x):
    """What MIOpen's choice of a convolution solver depends on, as far as a caller can see it."""
    return tuple(x.shape), torch.backends.cudnn.benchmark, torch.backends.cudnn.deterministic


class _Site:
    """One BatchNorm2d of the model: which epilogues were proven bit-equal on it, or that it was dropped."""

    __slots__ = ("bn", "verified", "dropped", "no_pool")

    def __init__(self, bn: nn.BatchNorm2d):
        self.bn = bn
        self.verified: set = set()
        self.dropped = False
        self.no_pool = False  # the pooled epilogue failed its proof here (the others may stand)

    def eligible(self, x) -> bool:
        if not _streamable(x) or not 0 < x.numel() <= N.BN_MAX_ELEMENTS or x.shape[1] > N.BN_MAX_CHANNELS:
            return False
        return self.usable(x.device, x.shape[1])

    def usable(self, device, channels: int) -> bool:
        """Everything of ``eligible`` that does not need the norm's input (K27 never holds it)."""
        bn = self.bn
        if self.dropped or bn.training or torch.is_grad_enabled() or not enabled():
            return False
        if not torch.backends.cudnn.enabled or torch.is_autocast_enabled():  # another BatchNorm kernel would have run
            return False
        for p in (bn.running_mean, bn.running_var, bn.weight, bn.bias):
            if p is None or p.dtype is not torch.float32 or p.device != device or not p.is_contiguous() or p.numel() != channels:
                return False
        return True

    def run(self, x, relu: bool, other=None, bn_first: bool = True):
        bn = self.bn
        out = N.batchnorm_infer(x, bn.running_mean, bn.running_var, bn.weight, bn.bias, bn.eps, relu=relu, residual=other)
        key = (relu, other is not None, (x.shape[2] * x.shape[3]) % 4 == 0)
        if key in self.verified:
            return out
        ref = F.batch_norm(x, bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0, bn.eps)
        if other is not None:
            ref = ref + other if bn_first else other + ref
        if relu:
            ref = torch.relu_(ref)
        if torch.equal(out.view(torch.int32), ref.view(torch.int32)):
            self.verified.add(key)
            return out
        self.dropped = True
        warnings.warn(
            f"the fused BatchNorm kernel did not reproduce PyTorch's result bit for bit on a {tuple(x.shape)} input "
            f"(relu={relu}, residual={other is not None}); this BatchNorm2d runs unfused from now on.", RuntimeWarning, stacklevel=3)
        return ref

    def pool_eligible(self, x, params) -> bool:
        (kh, kw), _, (ph, pw) = params
        return (not self.no_pool and x.shape[3] <= N.BN_POOL_MAX_WIDTH and x.shape[2] + 2 * ph >= kh
                and x.shape[3] + 2 * pw >= kw)

    def run_pool(self, x, params):
        bn = self.bn
        k, s, p = params
        out = N.batchnorm_infer_relu_maxpool(x, bn.running_mean, bn.running_var, bn.weight, bn.bias, bn.eps, k, s, p)
        banded = x.shape[2] > N.BN_POOL_STAGE_BYTES // (4 * x.shape[3])  # the launch that splits a plane into bands of rows
        key = ("pool", params, x.shape[3] % 4 == 0 and out.shape[3] % 4 == 0, banded)
        if key in self.verified:
            return out
        ref = F.batch_norm(x, bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0, bn.eps)
        ref = F.max_pool2d(torch.relu_(ref), k, s, p)
        if out.shape == ref.shape and torch.equal(out.view(torch.int32), ref.view(torch.int32)):
            self.verified.add(key)
            return out
        self.no_pool = True
        warnings.warn(
            f"the fused BatchNorm + ReLU + max-pool kernel did not reproduce PyTorch's result bit for bit on a {tuple(x.shape)} "
            f"input (kernel_size={k}, stride={s}, padding={p}); this max-pool runs unfused from now on.", RuntimeWarning,
            stacklevel=3)
        return ref


def _bn_args(bn: nn.BatchNorm2d):
    return bn.running_mean, bn.running_var, bn.weight, bn.bias, bn.eps


def _bn_forward(site: _Site):
    def forward(x):
        if site.eligible(x):
            return site.run(x, relu=False)
        return _BN_FORWARD(site.bn, x)

    return forward


class _Fused(nn.Module):
    """``relu(bn(x))`` or ``relu(add(bn(x), other))`` as one call; the modules themselves when the call is not eligible."""

    def __init__(self, site: _Site, relu, add=None, bn_first: bool = True):
        super().__init__()
        self.__dict__.update(site=site, relu=relu, add=add, bn_first=bn_first)  # (not registered as children)

    def forward(self, x, other=None):
        site, relu = self.site, self.relu
        ok = not _hooked(site.bn) and not (isinstance(relu, nn.Module) and _hooked(relu)) and site.eligible(x)
        if ok and self.add is not None:
            ok = _streamable(other) and other.shape == x.shape and other.device == x.device
        if ok:
            return site.run(x, relu=True, other=other, bn_first=self.bn_first)
        out = site.bn(x)
        if self.add is not None:
            out = self.add(out, other) if self.bn_first else self.add(other, out)
        return relu(out)


class _FusedDual(nn.Module):
    """``relu(add(bn(x), shortcut_bn(xb)))`` as one call: ``single`` is the fused tail of ``bn`` alone, ``seq`` the shortcut
    ``nn.Sequential`` whose last child is ``shortcut.bn`` and whose leading children the graph has called to produce ``xb``."""

    def __init__(self, single: _Fused, shortcut: _Site, seq: nn.Sequential):
        super().__init__()
        self.__dict__.update(single=single, shortcut=shortcut, seq=seq, children_seen=tuple(seq.children()), verified=set(),
                             dropped=False)  # (not registered as children)

    def ready(self) -> bool:
        """What is known before the owner runs: the graph that bypasses ``seq.__call__`` may be taken."""
        single, relu, now = self.single, self.single.relu, tuple(self.seq.children())
        return (not self.dropped and not _hooked(self.seq) and not _hooked(self.shortcut.bn) and not _hooked(single.site.bn)
                and not (isinstance(relu, nn.Module) and _hooked(relu)) and len(now) == len(self.children_seen)
                and all(a is b for a, b in zip(now, self.children_seen)))

    def forward(self, x, xb):
        a, b = self.single.site, self.shortcut
        if (self.ready() and a.eligible(x) and b.eligible(xb) and xb.shape == x.shape and xb.device == x.device
                and x.shape[1] <= N.BN_DUAL_MAX_CHANNELS):
            return self.run(x, xb)
        return self.single(x, b.bn(xb))  # the shortcut's norm as a module, then the tail of the first graph

    def run(self, x, xb):
        bn_first = self.single.bn_first
        left, right = ((x, self.single.site.bn), (xb, self.shortcut.bn)) if bn_first else ((xb, self.shortcut.bn), (x, self.single.site.bn))
        out = N.batchnorm_infer_add_bn_relu(left[0], _bn_args(left[1]), right[0], _bn_args(right[1]))
        key = ((x.shape[2] * x.shape[3]) % 4 == 0, bn_first)
        if key in self.verified:
            return out
        ref = torch.relu_(F.batch_norm(left[0], *_bn_args(left[1])[:4], False, 0.0, left[1].eps)
                          + F.batch_norm(right[0], *_bn_args(right[1])[:4], False, 0.0, right[1].eps))
        if torch.equal(out.view(torch.int32), ref.view(torch.int32)):
            self.verified.add(key)
            return out
        self.dropped = True
        warnings.warn(
            f"the fused BatchNorm + BatchNorm + add + ReLU kernel did not reproduce PyTorch's result bit for bit on {tuple(x.shape)} "
            f"inputs; this shortcut's BatchNorm2d runs on its own from now on.", RuntimeWarning, stacklevel=3)
        return ref


def _unhooked_tail(single: _Fused) -> bool:
    relu = single.relu
    return not _hooked(single.site.bn) and not (isinstance(relu, nn.Module) and _hooked(relu))


class _FusedConv(nn.Module):
    """``relu(add(bn(conv(x)), other))`` as one call.  ``single`` is the fused tail of ``bn`` alone, which takes
    the convolution's output when the call is not eligible: the convolution is then called as the module it is."""

    def __init__(self, single: _Fused, conv: nn.Conv2d):
        super().__init__()
        self.__dict__.update(single=single, conv=conv, verified=set(), dropped=False)  # (not registered as children)

    def ready(self) -> bool:
        """What is known before the owner runs: the graph that does not call ``conv`` may be taken."""
        return (conv_enabled() and not self.dropped and _tail_conv(self.conv) and not _hooked(self.conv)
                and _unhooked_tail(self.single))

    def forward(self, x, other):
        site = self.single.site
        if (self.ready() and _conv_operands(self.conv, x) and site.usable(x.device, N.CONV_TAIL_OUT) and _streamable(other)
                and other.device == x.device
                and tuple(other.shape) == (x.shape[0], N.CONV_TAIL_OUT, x.shape[2], x.shape[3])):
            return self.run(x, other)
        return self.single(self.conv(x), other)

    def run(self, x, other):
        bn, w, bn_first = self.single.site.bn, self.conv.weight, self.single.bn_first
        out = N.conv1x1_bn_add_relu(x, w, _bn_args(bn), other)
        key = (_solver_key(x), bn_first)
        if key in self.verified:
            return out
        ref = F.batch_norm(F.conv2d(x, w), *_bn_args(bn)[:4], False, 0.0, bn.eps)
        ref = torch.relu_(ref + other if bn_first else other + ref)
        if torch.equal(out.view(torch.int32), ref.view(torch.int32)):
            self.verified.add(key)
            return out
        self.dropped = True
        warnings.warn(
            f"the fused convolution + BatchNorm + add + ReLU kernel did not reproduce PyTorch's result bit for bit on a "
            f"{tuple(x.shape)} input; this convolution runs on its own from now on.", RuntimeWarning, stacklevel=3)
        return ref


class _FusedConvDual(nn.Module):
    """``relu(add(bn(conv(x)), shortcut_bn(shortcut_conv(xb))))`` as one call: ``dual`` is the K19 tail of the
    two norms, which takes the two convolutions' outputs when the call is not eligible."""

    def __init__(self, dual: _FusedDual, conv: nn.Conv2d, shortcut_conv: nn.Conv2d):
        super().__init__()
        self.__dict__.update(dual=dual, conv=conv, shortcut_conv=shortcut_conv, verified=set(), dropped=False)

    def ready(self) -> bool:
        return (conv_enabled() and not self.dropped and self.dual.ready() and len(self.dual.children_seen) == 2
                and self.dual.children_seen[0] is self.shortcut_conv and _tail_conv(self.conv) and _tail_conv(self.shortcut_conv)
                and not _hooked(self.conv) and not _hooked(self.shortcut_conv))

    def forward(self, x, xb):
        a, b = self.dual.single.site, self.dual.shortcut
        if (self.ready() and _conv_operands(self.conv, x) and _conv_operands(self.shortcut_conv, xb) and xb.shape == x.shape
                and xb.device == x.device and a.usable(x.device, N.CONV_TAIL_OUT) and b.usable(x.device, N.CONV_TAIL_OUT)):
            return self.run(x, xb)
        return self.dual(self.conv(x), self.shortcut_conv(xb))

    def run(self, x, xb):
        single, bn_first = self.dual.single, self.dual.single.bn_first
        ours, theirs = (x, self.conv.weight, single.site.bn), (xb, self.shortcut_conv.weight, self.dual.shortcut.bn)
        left, right = (ours, theirs) if bn_first else (theirs, ours)
        out = N.conv1x1_bn_add_conv1x1_bn_relu(left[0], left[1], _bn_args(left[2]), right[0], right[1], _bn_args(right[2]))
        key = (_solver_key(x), bn_first)
        if key in self.verified:
            return out
        ref = torch.relu_(F.batch_norm(F.conv2d(left[0], left[1]), *_bn_args(left[2])[:4], False, 0.0, left[2].eps)
                          + F.batch_norm(F.conv2d(right[0], right[1]), *_bn_args(right[2])[:4], False, 0.0, right[2].eps))
        if torch.equal(out.view(torch.int32), ref.view(torch.int32)):
            self.verified.add(key)
            return out
        self.dropped = True
        warnings.warn(
            f"the fused kernel of two convolutions, their BatchNorms, add and ReLU did not reproduce PyTorch's result bit for bit "
            f"on {tuple(x.shape)} inputs; these convolutions run on their own from now on.", RuntimeWarning, stacklevel=3)
        return ref


class _FusedPool(nn.Module):
    """``max_pool2d(relu(bn(x)))`` as one call.  ``pool`` is the user's ``nn.MaxPool2d`` or, for ``F.max_pool2d`` with literal
    arguments, their dict.  A call that is not eligible runs ``inner`` (the fused ``relu(bn(x))``, which steps aside on its own
    terms) and then the user's pool."""

    def __init__(self, inner: _Fused, pool):
        super().__init__()
        self.__dict__.update(inner=inner, pool=pool)  # (not registered as children)

    def forward(self, x):
        inner, pool = self.inner, self.pool
        site, relu = inner.site, inner.relu
        if isinstance(pool, nn.Module):  # parameters are read now: the user may have changed them since the trace
            params = _pool_params(*(getattr(pool, name) for name in _POOL_ARGS))
            hooked = _hooked(pool)
        else:
            params, hooked = _pool_params(**pool), False
        if (params is not None and not hooked and not _hooked(site.bn) and not (isinstance(relu, nn.Module) and _hooked(relu))
                and site.eligible(x) and site.pool_eligible(x, params)):
            return site.run_pool(x, params)
        out = inner(x)
        return pool(out) if isinstance(pool, nn.Module) else F.max_pool2d(out, **pool)


def _trace(parent: nn.Module, sites: dict, dual: bool = False, conv: bool = False):
    """GraphModule of ``parent``'s own forward with the fused patterns rewritten, or None.  ``dual``: also take a shortcut
    Sequential's BatchNorm into the tail call; then ``(GraphModule, [its _FusedDual modules])``, or None when there is none.
    ``conv``: also take a 64 -> 256 pointwise convolution in front of a residual tail into the call (and the shortcut's, where
    ``dual`` found a ``Sequential(conv, bn)``); then ``(GraphModule, [every module of it that has a ready()])``, or None when
    no convolution was taken."""
    from torch import fx

    class InplaceProxy(fx.Proxy):  # fx turns `a += b` into `a + b`; the graph must keep writing into `a`, which a caller may hold
        pass

    for name in ("iadd", "isub", "imul", "itruediv"):
        op = getattr(operator, name)
        setattr(InplaceProxy, f"__{name}__",
                lambda self, other, op=op: self.tracer.create_proxy("call_function", op, (self, other), {}))

    class LeafTracer(fx.Tracer):
        def is_leaf_module(self, m, qualname):
            return True

        def proxy(self, node):
            return InplaceProxy(node, self)

    params = list(inspect.signature(parent.forward).parameters.values())
    if any(p.kind is not p.POSITIONAL_OR_KEYWORD or p.default is not p.empty for p in params):
        return None  # a trace would freeze whatever the defaults or **kwargs select
    graph = LeafTracer().trace(parent)
    gm = fx.GraphModule(parent, graph)
    mods = dict(parent.named_modules())

    def relu_of(node):
        if node.kwargs or len(node.args) != 1:
            return None
        if node.op == "call_module" and _plain_relu(mods.get(node.target)):
            return mods[node.target]
        if node.op == "call_function" and node.target in _RELUS:
            return F.relu
        return None

    def pool_of(node, source):
        """The user's pool module, or the keyword form of a literal ``F.max_pool2d`` call, when ``node`` pools ``source``."""
        if not node.args or node.args[0] is not source:
            return None
        if node.op == "call_module" and _plain_pool(mods.get(node.target)) and len(node.args) == 1 and not node.kwargs:
            return mods[node.target]
        if node.op == "call_function" and node.target is F.max_pool2d and len(node.args) <= 1 + len(_POOL_ARGS):
            given = dict(zip(_POOL_ARGS, node.args[1:]))
            if set(given) & set(node.kwargs) or not set(node.kwargs) <= set(_POOL_ARGS):
                return None
            given.update(node.kwargs)
            flat = [e for v in given.values() for e in (v if isinstance(v, (tuple, list)) else (v,))]
            if "kernel_size" in given and not any(isinstance(e, fx.Node) for e in flat):
                return given
        return None

    def shortcut_of(node, add):
        """The site of the trailing BatchNorm2d when ``node`` calls a plain Sequential whose only consumer is ``add``."""
        seq = mods.get(node.target) if node.op == "call_module" else None
        if not _plain_seq(seq) or node.kwargs or len(node.args) != 1 or set(node.users) != {add}:
            return None
        children = list(seq.children())
        return sites.get(children[-1]) if len(children) >= 2 else None

    def conv_of(node, consumer):
        """The convolution when ``node`` calls one the K27 kernels compute and ``consumer`` is all that reads its output."""
        m = mods.get(node.target) if isinstance(node, fx.Node) and node.op == "call_module" else None
        if not _tail_conv(m) or node.kwargs or len(node.args) != 1 or set(node.users) != {consumer}:
            return None
        return m

    n_fused, duals, convs = 0, [], []
    for node in list(graph.nodes):
        if node.op != "call_module" or mods.get(node.target) not in sites or node.kwargs or len(node.args) != 1:
            continue
        if len(node.users) != 1:
            continue
        site, user = sites[mods[node.target]], next(iter(node.users))
        last, fused, args, stale = user, None, None, []
        if relu_of(user) is not None:
            fused, args = _Fused(site, relu_of(user)), (node.args[0],)
            follower = next(iter(user.users)) if len(user.users) == 1 else None  # the pool must be the ReLU's only consumer
            pool = pool_of(follower, user) if follower is not None else None
            if pool is not None:
                last, fused = follower, _FusedPool(fused, pool)
        elif (user.op == "call_function" and user.target in _ADDS and not user.kwargs and len(user.args) == 2
              and all(isinstance(a, fx.Node) for a in user.args) and user.args[0] is not user.args[1] and len(user.users) == 1):
            last = next(iter(user.users))
            if relu_of(last) is None:
                continue
            bn_first = user.args[0] is node
            if user.target is operator.iadd and not bn_first:
                continue  # `other += bn(x)` writes into `other`, which the caller may hold: not the fused call's fresh tensor
            fused = _Fused(site, relu_of(last), user.target, bn_first)
            other = user.args[1] if bn_first else user.args[0]
            args = (node.args[0], other)
            shortcut = shortcut_of(other, user) if dual else None
            if shortcut is not None:
                # the leading children where the Sequential was called (a block may run its shortcut before its first conv),
                # each through its own __call__; only the BatchNorm moves into the tail
                seq, tail = mods[other.target], other.args[0]
                with graph.inserting_before(other):
                    for child_name in list(seq._modules)[:-1]:
                        tail = graph.call_module(f"{other.target}.{child_name}", (tail,))
                fused, args, stale = _FusedDual(fused, shortcut, seq), (node.args[0], tail), [other]
                duals.append(fused)
            ours = conv_of(node.args[0], node) if conv else None
            if ours is not None and isinstance(fused, _Fused):
                fused, args, stale = _FusedConv(fused, ours), (node.args[0].args[0], other), [node.args[0]]
                convs.append(fused)
            elif ours is not None and isinstance(fused, _FusedDual) and len(fused.children_seen) == 2 and _tail_conv(
                    fused.children_seen[0]):
                # K19's rewrite above called the shortcut's convolution where the Sequential was (args[1]); that call and
                # conv3's leave the graph
                duals.remove(fused)
                stale += [node.args[0], args[1]]
                fused, args = _FusedConvDual(fused, ours, fused.children_seen[0]), (node.args[0].args[0], other.args[0])
                convs.append(fused)
        if fused is None:
            continue
        name = f"_sl_fused_{n_fused}"
        n_fused += 1
        gm.add_submodule(name, fused)
        with graph.inserting_before(last):
            new = graph.call_module(name, args)
        last.replace_all_uses_with(new)
        graph.erase_node(last)
        if last is not user:
            graph.erase_node(user)
        graph.erase_node(node)
        for dead in stale:
            graph.erase_node(dead)
    if not n_fused or (conv and not convs) or (dual and not conv and not duals):
        return None
    graph.lint()
    gm.recompile()
    if conv:
        return gm, convs + duals  # (a K19 tail that stands on its own in this graph gates it too)
    return (gm, duals) if dual else gm


def _owner_forward(parent: nn.Module, gm, training: bool, dual=None, conv=None):
    """The traced forward while the owner is in the mode it was traced in (a trace freezes `if self.training:`), its own otherwise.
    ``dual``: the graph that also fuses a shortcut's BatchNorm and its ``_FusedDual`` modules; taken when all of them are ready.
    ``conv``: the graph that also fuses the tail's convolutions, likewise, and first."""
    own = type(parent).forward

    def forward(*args, **kwargs):
        if parent.training is training:
            if conv is not None and all(f.ready() for f in conv[1]):
                return conv[0].forward(*args, **kwargs)
            if dual is not None and all(f.ready() for f in dual[1]):
                return dual[0].forward(*args, **kwargs)
            return gm.forward(*args, **kwargs)
        return own(parent, *args, **kwargs)

    return forward


class _Plan:
    def __init__(self, model: nn.Module):
        self.module_ids = tuple(id(m) for m in model.modules())
        self.sites = {m: _Site(m) for m in model.modules() if _plain_bn(m) and m is not model}
        self.parents: list = []  # (weak reference to the owner, GraphModule, the owner's training flag when it was traced)
        self.duals: dict = {}  # index into `parents` -> (GraphModule with the shortcut's BatchNorm in the tail, its _FusedDual modules)
        self.convs: dict = {}  # index into `parents` -> (GraphModule with the tail's convolutions in it, the modules that gate it)
        for parent in model.modules():
            if "forward" in parent.__dict__ or not any(child in self.sites for child in parent.children()):
                continue
            try:
                gm = _trace(parent, self.sites)
            except Exception:  # control flow on tensor values, *args, ...: this module keeps its own forward
                gm = None
            if gm is None:
                continue
            self.parents.append((weakref.ref(parent), gm, parent.training))
            if any(_plain_seq(c) and len(c) >= 2 and c[-1] in self.sites for c in parent.children()):
                try:
                    dual = _trace(parent, self.sites, dual=True)
                except Exception:
                    dual = None
                if dual is not None:
                    self.duals[len(self.parents) - 1] = dual
            if any(_tail_conv(c) for c in parent.children()):
                try:
                    conv = _trace(parent, self.sites, dual=len(self.parents) - 1 in self.duals, conv=True)
                except Exception:
                    conv = None
                if conv is not None:
                    self.convs[len(self.parents) - 1] = conv

    def valid_for(self, model: nn.Module) -> bool:
        return self.module_ids == tuple(id(m) for m in model.modules())


def substitute(model: nn.Module):
    """Install the fused forwards on ``model``; returns the function that removes them (None when switched off)."""
    if not enabled() or not isinstance(model, nn.Module):
        return None
    plan = _PLANS.get(model)
    if plan is None or not plan.valid_for(model):
        plan = _PLANS[model] = _Plan(model)
    swapped = []
    for bn, site in plan.sites.items():
        if "forward" not in bn.__dict__:
            bn.forward = _bn_forward(site)
            swapped.append(bn)
    for i, (ref, gm, training) in enumerate(plan.parents):
        parent = ref()
        if parent is not None and "forward" not in parent.__dict__:
            parent.forward = _owner_forward(parent, gm, training, plan.duals.get(i), plan.convs.get(i))
            swapped.append(parent)

    def undo():
        for m in swapped:
            m.__dict__.pop("forward", None)
        swapped.clear()

    return undo
