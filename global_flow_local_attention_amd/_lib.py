"""ctypes binding of libgfla_hip.so.

include/gfla_hip.h is the single description of the C ABI: the argument and return types of every entry point, the
dispatch-trace ids (enum gfla_path -> PATH_*), the tuning keys (enum gfla_tuning_key -> TUNE_*), the status codes and
ABI_VERSION are read from it, never restated here.
Headers it includes (include/gfla_gen_conv.h, include/gfla_lds_plane.h, include/gfla_spectral_norm.h,
include/gfla_conv3d.h, include/gfla_adam.h, include/gfla_pose.h, include/gfla_image.h, include/gfla_metrics.h) are read in
the same way.

The library is the only implementation of the ops: there is no Python/torch fallback.  If it
is missing or fails to load, importing an op raises; if a call returns a non-zero status, a
RuntimeError is raised (the reference swallows native errors, block_extractor_cuda.cc:11).
"""
import contextlib
import ctypes
import os
import re
import subprocess

import torch

_PKG = os.path.dirname(os.path.abspath(__file__))
# GFLA_HIP_LIBRARY: a differently built library (tools/ubench/build_agg_abl.sh timing variants); default = the in-tree build
LIB_PATH = os.environ.get("GFLA_HIP_LIBRARY") or os.path.join(_PKG, "libgfla_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_PKG), "include", "gfla_hip.h")   # csrc/Makefile: ../../include/gfla_hip.h
# headers gfla_hip.h includes, in the same dialect: their entry points are bound as well (extension_symbols)
EXTENSION_HEADER_PATHS = tuple(os.path.join(os.path.dirname(HEADER_PATH), name) for name in ("gfla_gen_conv.h", "gfla_lds_plane.h",
                                                                                            "gfla_spectral_norm.h", "gfla_conv3d.h", "gfla_adam.h", "gfla_pose.h",
                                                                                            "gfla_image.h", "gfla_metrics.h"))
_lib = None

# the types the ABI is written in; a pointer of any pointee crosses as c_void_p
_ARG_TYPES = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double, "gfla_stream_t": ctypes.c_void_p}
_RETURN_TYPES = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "const char *": ctypes.c_char_p}


def _enum_items(body, decl):
    for item in filter(None, (i.strip() for i in body.split(","))):
        m = re.fullmatch(r"(\w+) = (-?\d+)", item)
        if m is None:
            raise ValueError("gfla_hip.h: enumerator without an explicit integer value: %r in %r" % (item, decl))
        yield m.group(1), int(m.group(2))


def parse_header(text):
    """(functions, constants) of a header in gfla_hip.h's dialect.  functions: entry point -> (restype, [argtypes]), with
    every GFLA_DECL_*(SFX, T) instantiation expanded; constants: enumerators and integer #defines -> int.  Strict: a type
    outside _ARG_TYPES / _RETURN_TYPES, or a statement that is no declaration, typedef or enum, raises ValueError with the
    declaration in its message."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S).replace("\\\n", " ")
    functions, constants, macros, code = {}, {}, {}, []
    for line in text.splitlines():
        line = line.strip()
        m = re.match(r"#\s*define\s+(\w+)(\(SFX, T\))?\s*(.*)", line)
        if m and m.group(2):
            macros[m.group(1)] = m.group(3)
        elif m and re.fullmatch(r"-?\d+", m.group(3)):
            constants[m.group(1)] = int(m.group(3))
        elif not line.startswith("#") and line not in ('extern "C" {', "}"):   # include guard, #undef, the C++ wrapper
            code.append(line)
    code = re.sub(r"\b(GFLA_DECL_\w+)\((\w+), (\w+)\)",
                  lambda m: re.sub(r"\bT\b", m.group(3), macros[m.group(1)].replace("##SFX", m.group(2))), " ".join(code))
    for decl in filter(None, (" ".join(d.split()) for d in code.split(";"))):
        enum = re.fullmatch(r"(?:typedef )?enum \w+ \{(.*)\}(?: \w+)?", decl)
        if enum:
            constants.update(_enum_items(enum.group(1), decl))
            continue
        if re.fullmatch(r"typedef void \*gfla_stream_t", decl):
            continue
        m = re.fullmatch(r"(.*?)(gfla_\w+)\((.*)\)", decl)
        if m is None:
            raise ValueError("gfla_hip.h: not a declaration this binding understands: %r" % decl)
        ret, name, args = m.group(1).strip(), m.group(2), m.group(3).strip()
        if ret not in _RETURN_TYPES:
            raise ValueError("gfla_hip.h: unknown return type %r in %r" % (ret, decl))
        argtypes = []
        for arg in ([] if args == "void" else args.split(",")):
            ctype = re.sub(r"\w+$", "", arg.strip()).strip()     # drop the parameter's name
            if "*" in ctype:
                argtypes.append(ctypes.c_void_p)
            elif ctype in _ARG_TYPES:
                argtypes.append(_ARG_TYPES[ctype])
            else:
                raise ValueError("gfla_hip.h: unknown argument type %r (%r) in %r" % (ctype, arg.strip(), decl))
        functions[name] = (_RETURN_TYPES[ret], argtypes)
    return functions, constants


def _read_header(path=HEADER_PATH):
    if not os.path.exists(path):
        raise RuntimeError("include/%s, the description of the C ABI, is missing (%s)" % (os.path.basename(path), path))
    with open(path) as f:
        return parse_header(f.read())


_FUNCTIONS, _CONSTANTS = _read_header()   # once per process
_EXTENSION_FUNCTIONS = {}
for _path in EXTENSION_HEADER_PATHS:
    _EXTENSION_FUNCTIONS.update(_read_header(_path)[0])
ABI_VERSION = _CONSTANTS["GFLA_ABI_VERSION"]
_ERR_UNSUPPORTED = _CONSTANTS["GFLA_ERR_UNSUPPORTED"]
# dispatch-trace ids: GFLA_PATH_X of enum gfla_path is PATH_X here (PATH_BE_BWD_LDS ... PATH_COUNT)
globals().update((name[len("GFLA_"):], value) for name, value in _CONSTANTS.items() if name.startswith("GFLA_PATH_"))
# tuning keys: GFLA_TUNE_X of enum gfla_tuning_key is TUNE_X here; the header says what each selects and who reads it
TUNING_KEYS = {name[len("GFLA_"):]: value for name, value in _CONSTANTS.items() if name.startswith("GFLA_TUNE_")}
globals().update(TUNING_KEYS)


def exported_symbols():
    """Every symbol include/gfla_hip.h declares."""
    return list(_FUNCTIONS)


def extension_symbols():
    """Every symbol the headers included by gfla_hip.h declare (EXTENSION_HEADER_PATHS)."""
    return list(_EXTENSION_FUNCTIONS)


def build(force=False):
    """Compile csrc/*.hip for gfx950 into libgfla_hip.so (hipcc cross-compiles without a GPU)."""
    cmd = ["make", "-C", os.path.join(_PKG, "csrc"), "-j8"]
    if force:
        cmd.append("-B")
    subprocess.check_call(cmd, stdout=subprocess.DEVNULL)
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "libgfla_hip.so is not built (%s). Run `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C global_flow_local_attention_amd/csrc`. There is no fallback path." % LIB_PATH)
        handle = ctypes.CDLL(LIB_PATH)
        for name, (restype, argtypes) in list(_FUNCTIONS.items()) + list(_EXTENSION_FUNCTIONS.items()):
            fn = getattr(handle, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib = handle
    return _lib


SUFFIX = {torch.float32: "f32", torch.float64: "f64", torch.bfloat16: "bf16", torch.float16: "f16"}
# 16-bit storage types: fp32 arithmetic inside, reductions over channels in float32
HALF_TYPES = (torch.bfloat16, torch.float16)


def suffix(t, what):
    """Entry-point suffix for t's dtype."""
    try:
        return SUFFIX[t.dtype]
    except KeyError:
        raise TypeError("%s: unsupported dtype %s (float32, float64, bfloat16, float16)" % (what, t.dtype))


IMPLS = ("auto", "torch")


def check_impl(impl):
    if impl not in IMPLS:
        raise ValueError("impl: one of %s (got %r)" % (IMPLS, impl))


def reduction_like(t):
    """Zeroed buffer for a gradient that is a reduction over channels (grad_flow, grad_logits, grad_in2): float32 when the
    storage type is 16-bit (the bf16 / f16 backward entry points accumulate these in float32), t's dtype otherwise."""
    return torch.zeros(t.shape, dtype=torch.float32 if t.dtype in HALF_TYPES else t.dtype, device=t.device)


def workspace_bytes(query_name, *sizes, what):
    """Answer of the `*_bytes` size query `query_name` for `sizes`.  A negative answer is a gfla_status: Unsupported for
    GFLA_ERR_UNSUPPORTED (callers with another way to the result catch it), ValueError for anything else."""
    n = int(getattr(lib(), query_name)(*(int(s) for s in sizes)))
    if n < 0:
        err = Unsupported if n == _ERR_UNSUPPORTED else ValueError
        raise err("%s%s: %s" % (what, tuple(int(s) for s in sizes), lib().gfla_status_string(n).decode()))
    return n


def workspace(query_name, ref_tensor, *sizes, what):
    """Scratch of the size `query_name` asks for, on ref_tensor's device: at least 16 bytes, so never a NULL pointer."""
    return torch.empty(max(workspace_bytes(query_name, *sizes, what=what), 16), dtype=torch.uint8, device=ref_tensor.device)


def scatter_workspace(ref_tensor, B, H, W, entries):
    """Scratch for the matrix-core scatter paths (csrc/patch_mfma.hip): the patch table of one op invocation."""
    return workspace("gfla_scatter_workspace_bytes", ref_tensor, B, H, W, entries, what="scatter workspace")


def aggregate_fwd(source, flow, logits, out, attn, k, apply_softmax):
    """softmax + aggregate forward.  f32 / bf16 / f16 storage: the coefficient-table kernels (scratch from the caching
    allocator, csrc/local_attn_aggregate.hip); f64: the plain entry point."""
    b, c, hs, ws = source.shape
    h, w = flow.shape[2], flow.shape[3]
    sfx = suffix(source, "local_attn_aggregate")
    tail = (b, c, hs, ws, h, w, int(k), 1 if apply_softmax else 0)
    if sfx in ("f32", "bf16", "f16"):
        scratch = workspace("gfla_aggregate_fwd_workspace_bytes", source, b, h, w, k, what="local_attn_aggregate")
        call("gfla_local_attn_aggregate_fwd_ws_" + sfx, source, ptr(source), ptr(flow), ptr(logits), ptr(out), ptr(attn),
             ptr(scratch), *tail)
    else:
        call("gfla_local_attn_aggregate_fwd_" + sfx, source, ptr(source), ptr(flow), ptr(logits), ptr(out), ptr(attn), *tail)


def require_gpu(*tensors):
    """The reference raises NotImplementedError for non-CUDA tensors (block_extractor.py:23-24)."""
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise NotImplementedError("GFLA ops run on the GPU only (got a %s tensor); there is no CPU path"
                                      % t.device.type)


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class Unsupported(RuntimeError):
    """GFLA_ERR_UNSUPPORTED (-3): the arguments are valid but outside what this entry point's kernels take (nothing was
    launched).  Callers that have another way to the same result catch exactly this."""


def call(name, ref_tensor, *args):
    """Invoke `name` on the current stream of ref_tensor's device; raise on non-zero status."""
    fn = getattr(lib(), name)
    with torch.cuda.device(ref_tensor.device):
        stream = ctypes.c_void_p(torch.cuda.current_stream(ref_tensor.device).cuda_stream)
        status = fn(*args, stream)
    if status != 0:
        err = Unsupported if status == _ERR_UNSUPPORTED else RuntimeError
        raise err("%s failed: %s (status %d)" % (name, lib().gfla_status_string(status).decode(), status))


# gfla_convert_multi's flag per (from, to) pair
_CONVERT_FLAG = {(torch.bfloat16, torch.float32): 0, (torch.float32, torch.bfloat16): 1,
                 (torch.float16, torch.float32): 2, (torch.float32, torch.float16): 3}


def convert_many(tensors, dtype):
    """[t.to(dtype) for t in tensors] for bfloat16 / float16 <-> float32 CUDA tensors, up to four per launch
    (gfla_convert_multi); None entries pass through.  Anything else (other dtypes, CPU tensors, nothing to convert) goes to
    torch."""
    out = list(tensors)
    todo = [i for i, t in enumerate(out) if t is not None and t.dtype != dtype]
    pair_ok = all(out[i].is_cuda and (out[i].dtype, dtype) in _CONVERT_FLAG for i in todo)
    if not todo or not pair_ok or len({out[i].dtype for i in todo}) != 1:
        return [None if t is None else t.to(dtype) for t in out]
    flag = _CONVERT_FLAG[(out[todo[0]].dtype, dtype)]
    for at in range(0, len(todo), 4):
        grp = todo[at:at + 4]
        srcs = [out[i].contiguous() for i in grp]
        dsts = [torch.empty(t.shape, dtype=dtype, device=t.device) for t in srcs]
        args = []
        for j in range(4):
            args += [ptr(srcs[j]), ptr(dsts[j]), srcs[j].numel()] if j < len(grp) else [None, None, 0]
        call("gfla_convert_multi", srcs[0], *args, flag)
        for i, d in zip(grp, dsts):
            out[i] = d
    return out


def unfold_supported(Hs, Ws, k, elem_size):
    return bool(lib().gfla_unfold_supported(int(Hs), int(Ws), int(k), int(elem_size)))


def set_tuning(key, value):
    """Process-global tuning knob `key` (a TUNE_* of include/gfla_hip.h: enum gfla_tuning_key); returns the old value.
    ValueError for a key that is no enumerator: the library would accept it and do nothing."""
    if int(key) not in TUNING_KEYS.values():
        raise ValueError("set_tuning: %r is no tuning key of include/gfla_hip.h (enum gfla_tuning_key)" % (key,))
    return lib().gfla_set_tuning(int(key), int(value))


@contextlib.contextmanager
def tuned(keys):
    """with tuned({TUNE_X: value, ...}): the keys set for the block, their previous values back on every way out, in
    reverse order.  Nests."""
    old = []
    try:
        for key, value in keys.items():
            old.append((key, set_tuning(key, value)))
        yield
    finally:
        for key, value in reversed(old):
            set_tuning(key, value)


def fc_path(mode, backward=False):
    """Dispatch-trace id of gfla_fc_forward_f32 / gfla_fc_backward_f32 in arithmetic mode `mode` (modes 0-4: ids 2-6 / 7-11)."""
    if int(mode) == 5:
        return PATH_FC_BWD_MODE5 if backward else PATH_FC_FWD_MODE5
    return (PATH_FC_BWD_MODE0 if backward else PATH_FC_FWD_MODE0) + int(mode)


def path_count(path):
    """How many times kernel path `path` has been enqueued by this process (any host thread)."""
    return int(lib().gfla_path_count(int(path)))
