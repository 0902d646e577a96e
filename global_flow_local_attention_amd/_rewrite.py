"""What the in-place rewrites of a network share (gen_conv.py, head_conv.py, instance_norm.py, spectral_norm.py): the tests
on a slot's neighbours and on a module's hooks, the pass over second registrations, and the idempotent wrappers of the
reference's constructors and methods.  What each fuse_* function looks for is its own loop; only the mechanics are here."""
from torch import nn
from torch.nn.utils.spectral_norm import SpectralNorm as _TorchSpectralNorm


def is_reflect_pad(module):
    return type(module) is nn.ReflectionPad2d and tuple(module.padding) == (1, 1, 1, 1)


def slope_of(module, relu):
    """negative slope of an activation an op can absorb, else None: nn.LeakyReLU, and with `relu` nn.ReLU as slope 0"""
    if type(module) is nn.LeakyReLU:
        return float(module.negative_slope)
    if relu and type(module) is nn.ReLU:
        return 0.0
    return None


def no_hooks(module, but=()):
    """no hook of any kind on `module` (spectral norm recomputes the weight in one; any other would silently stop firing
    once the slot is replaced), the forward pre-hooks `but` apart"""
    pre = [h for h in module._forward_pre_hooks.values() if not any(h is b for b in but)]
    return not (pre or module._forward_hooks or module._backward_hooks or module._backward_pre_hooks)


def plain(module):
    """a module an op can stand in for: its own `weight` Parameter and no hook at all"""
    return "weight" in module._parameters and no_hooks(module)


def spectral_norm_hook(module, dims=(0,)):
    """the SpectralNorm hook object (name "weight", a dim of `dims`: 0, or 1 as torch picks for a transposed convolution)
    of a module that carries exactly that one hook, or None"""
    hooks = list(module._forward_pre_hooks.values())
    if len(hooks) != 1 or type(hooks[0]) is not _TorchSpectralNorm or not no_hooks(module, hooks):
        return None
    hook = hooks[0]
    if hook.name != "weight" or hook.dim not in dims or "weight_orig" not in module._parameters:
        return None
    return hook


def run_with_add(seq, x, add):
    """seq(x) with `add` handed to its last module"""
    mods = list(seq)
    for m in mods[:-1]:
        x = m(x)
    return mods[-1](x, add)


def epilogue_slot(seq):
    """the last module of the nn.Sequential `seq` when it adds a residual in its own epilogue -- its `fuses_add` is true:
    an InferenceConv, a SpectralConv on a kernel geometry, a SpectralConvTranspose on the transposed 3x3 kernels --, else
    None.  The residual forwards of every rewrite ask this one question."""
    if not isinstance(seq, nn.Sequential) or len(seq) == 0:
        return None
    last = seq[len(seq) - 1]
    return last if getattr(last, "fuses_add", False) else None


def replace_aliases(net, replaced):
    """`replaced`: id(old) -> (old, new).  Every other name an old module is registered under (the reference's Jump keeps
    its convolution as `conv1` and `model.N`) gets the same new module."""
    for m in net.modules():
        for name, sub in m._modules.items():
            if sub is not None and id(sub) in replaced and replaced[id(sub)][0] is sub:
                m._modules[name] = replaced[id(sub)][1]


def wrap_method(cls, name, flag, make):
    """Replace the method `name` that `cls` itself defines by make(original), marked with the attribute `flag` and with
    the original as __wrapped__; a method that carries the flag already stays.  False when cls is None or defines none."""
    orig = None if cls is None else cls.__dict__.get(name)
    if orig is None:
        return False
    if not getattr(orig, flag, False):
        new = make(orig)
        setattr(new, flag, True)
        new.__wrapped__ = orig
        new.__doc__ = orig.__doc__
        setattr(cls, name, new)
    return True


def wrap_init(cls, flag, after):
    """wrap_method for the constructor: after(self) runs on every finished instance"""
    def make(orig):
        def __init__(self, *args, **kwargs):
            orig(self, *args, **kwargs)
            after(self)
        return __init__
    return wrap_method(cls, "__init__", flag, make)
