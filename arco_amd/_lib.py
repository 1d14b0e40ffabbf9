"""ctypes binding of the C-ABI library arco_amd/lib/libarco_hip.so (include/arco_hip.h).

The product path has NO CPU fallback: every op below raises if the HIP extension
is missing or a launch fails.  PyTorch only owns memory and streams.
"""
import ctypes
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ARCO_LIB") or os.path.join(_HERE, "lib", "libarco_hip.so")     # ARCO_LIB: an A/B build (tools/build_variant.sh)
_lib = None

_P, _I, _L, _F, _U64, _D = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_uint64, ctypes.c_double
_SCALARS = {"int": _I, "long": _L, "float": _F, "double": _D, "uint64_t": _U64}      # every scalar type include/arco_hip.h uses; closed


def parse_header(text):
    """The binding tables from the text of include/arco_hip.h, which the compiler holds to the definitions (csrc/common.h includes it).
    -> (sigs, queries): sigs[name] = argtypes of an entry point whose last parameter is `void* stream` (int status; `call` appends the
    stream), queries[name] = (argtypes, restype) of every other one.  A parameter with `*` is c_void_p, a scalar goes through _SCALARS;
    anything the rules below cannot read raises - nothing is guessed."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)                        # comments
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)                               # preprocessor lines
    text = re.sub(r"\btypedef\s+struct\b[^{;]*\{.*?\}[^;]*;", " ", text, flags=re.S)    # ArcoActPro (mirrored by ActPro below)
    decls = re.findall(r"([^;{}()]*?)\b(arco_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text)
    names = set(re.findall(r"\b(arco_[a-z0-9_]+)\s*\(", text))
    if not decls or len(decls) != len(names):
        raise RuntimeError(f"arco_amd: arco_hip.h: {len(decls)} declarations read, {len(names)} arco_*( names present: "
                           f"{sorted(names - {d[1] for d in decls})}")
    sigs, queries = {}, {}
    for ret, name, params in decls:
        ret, params = " ".join(ret.split()), [" ".join(p.split()) for p in params.split(",")]
        if params in ([""], ["void"]):
            params = []
        args = []
        for p in params:
            ctype = p.rsplit(" ", 1)[0].replace("const ", "")                         # drop the parameter's name
            if "*" not in p and ctype not in _SCALARS:
                raise RuntimeError(f"arco_amd: arco_hip.h: {name}: parameter `{p}` has a type outside {sorted(_SCALARS)}")
            args.append(_P if "*" in p else _SCALARS[ctype])
        if ret != "void" and ret not in _SCALARS:
            raise RuntimeError(f"arco_amd: arco_hip.h: {name}: return type `{ret}` is outside {sorted(_SCALARS)} and void")
        if params and params[-1].replace(" ", "") == "void*stream":
            if ret != "int":
                raise RuntimeError(f"arco_amd: arco_hip.h: {name}: takes a stream, so it returns the int status, not `{ret}`")
            sigs[name] = args
        else:
            queries[name] = (args, None if ret == "void" else _SCALARS[ret])
    return sigs, queries


def read_header(path):
    if not os.path.exists(path):
        raise RuntimeError(f"arco_amd: the C-ABI header {path} is missing - the binding is derived from it")
    with open(path) as f:
        return parse_header(f.read())


HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "arco_hip.h")
_SIGS, _QUERIES = read_header(HEADER_PATH)      # name -> argtypes (int status); name -> (argtypes, restype) of the plain host helpers
EXPORTS = sorted(list(_SIGS) + list(_QUERIES))


def load():
    """Load the shared library (once).  Fails loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"arco_amd: HIP extension {LIB_PATH} is missing - build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` (make -C arco_amd/csrc). "
                "There is no CPU fallback.")
        lib = ctypes.CDLL(LIB_PATH)
        for name, args in _SIGS.items():
            fn = getattr(lib, name)
            fn.argtypes, fn.restype = args, _I
        for name, (args, res) in _QUERIES.items():
            fn = getattr(lib, name)
            fn.argtypes, fn.restype = args, res
        _lib = lib
    return _lib


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class ActPro(ctypes.Structure):
    """include/arco_hip.h ArcoActPro: the consumer-side activation descriptor of arco_conv3d_fwd_pro / arco_conv3d_wgrad_pro."""
    _fields_ = [("mean", _P), ("istd", _P), ("gamma", _P), ("beta", _P), ("slope", _F), ("groups", _I),
                ("drop_mode", _I), ("p", _F), ("seed", _U64), ("seed_dev", _P)]


def act_pro(mean, istd, gamma, beta, slope, groups, drop_mode, p, seed, seed_dev):
    d = ActPro(mean.data_ptr(), istd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), float(slope), int(groups), int(drop_mode),
               float(p), int(seed), None if seed_dev is None else seed_dev.data_ptr())
    return ctypes.byref(d)


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_raw_device = getattr(torch._C, "_cuda_getDevice", None)


def stream():
    """The current torch HIP stream of the current device as a hipStream_t.  torch.cuda.current_stream() costs
    ~9 us of Python per call (device-index plumbing); the raw accessors cost ~0.3 us - at ~500 launches per step
    that is 4 ms of host time."""
    if _raw_stream is not None and _raw_device is not None:
        return ctypes.c_void_p(_raw_stream(_raw_device()))
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def call(name, *args):
    """Invoke a kernel entry point on the current torch HIP stream; raise on error."""
    rc = getattr(load(), name)(*args, stream())
    if rc != 0:
        raise RuntimeError(f"arco_amd: {name} failed with code {rc}")


def query(name, *args):
    return getattr(load(), name)(*args)


def h(name, t):
    """Entry point `name`, or its `_h` form (f16 activation storage) where `t` - a tensor the call reads, or a bool - says f16."""
    half = t if isinstance(t, bool) else t is not None and t.dtype == torch.float16
    return name + "_h" if half else name


def require_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("arco_amd: tensors must live on the GPU (no CPU fallback); got a CPU tensor")
