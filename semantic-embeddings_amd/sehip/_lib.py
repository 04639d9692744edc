"""ctypes binding of libsehip.so, declared from its C ABI in include/sehip.h.

The header is the only statement of the ABI: ``parse_header`` reads its prototypes and integer ``#define``s, ``lib()`` declares
every entry point from them, and ``call`` checks every tensor against the element type of its pointer parameter.

The library is built in-tree by ``csrc/Makefile`` (``hipcc --offload-arch=gfx950``).  There is NO
CPU fallback: if the shared object is missing, or a kernel is asked to run without a ROCm device,
the call raises -- the product path never silently degrades to PyTorch/NumPy code.
"""
import collections
import ctypes
import os
import re
import subprocess

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(os.path.dirname(_HERE), "csrc")
HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "sehip.h")
LIB_PATH = os.environ.get("SEHIP_LIB") or os.path.join(_HERE, "libsehip.so")   # SEHIP_LIB: tuning builds only
TUNING_LIB_PATH = os.path.join(_HERE, "libsehip_tuning.so")   # -DSE_TUNING build: honours the SE_* variant / profile switches


class SehipError(RuntimeError):
    pass


Param = collections.namedtuple("Param", "ctype pointee name")     # pointee: element type of a pointer parameter, else None
Prototype = collections.namedtuple("Prototype", "restype params stream")   # stream: a trailing se_stream_t follows params

_SCALARS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "se_stream_t": ctypes.c_void_p}
_RESTYPES = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t, "const char *": ctypes.c_char_p}
# torch dtypes a tensor may have for a pointer to each element type (int16 / int32 carry the bit patterns of unsigned data)
_POINTEES = {"float": (torch.float32,), "double": (torch.float64,), "int32_t": (torch.int32,), "int64_t": (torch.int64,),
             "uint16_t": (torch.int16, torch.uint16), "uint32_t": (torch.int32, torch.uint32), "char *": (),
             "void": frozenset(v for v in vars(torch).values() if isinstance(v, torch.dtype))}


def _param(decl, where):
    """'const int64_t *labels' -> Param("int64_t *", "int64_t", "labels"); a type outside the map raises."""
    m = re.fullmatch(r"(?:const\s+)?(\w+)\s*((?:\*\s*)*)(\w*)", decl.strip())
    if m:
        base, stars = m.group(1), m.group(2).count("*")
        pointee = base + " *" * (stars - 1) if stars else None
        if (pointee in _POINTEES) if stars else (base in _SCALARS):
            return Param(base + " *" * stars, pointee, m.group(3))
    raise SehipError("%s: unsupported parameter type in %r" % (where, " ".join(decl.split())))


def parse_header(text):
    """-> ({name: Prototype} of every ``se_*`` function declared in ``text``, {name: value} of every integer ``#define SE_*``).
    A type outside the map this binding knows raises ``SehipError`` naming the declaration."""
    text = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))
    defines = {m.group(1): int(m.group(2).strip("()"))
               for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(SE_\w+)[ \t]+(-?\d+|\(-?\d+\))[ \t]*$", text, flags=re.M)}
    prototypes = {}
    for stmt in re.split(r"[;{}]", re.sub(r"^[ \t]*#[^\n]*", "", text, flags=re.M)):
        m = re.fullmatch(r"\s*([\w\s*]+?)\s*\b(se_\w+)\s*\(([^()]*)\)\s*", stmt)
        if not m:
            if re.search(r"\bse_\w+\s*\(", stmt):
                raise SehipError("cannot read the declaration %r" % " ".join(stmt.split()))
            continue
        where, restype, decls = m.group(2) + "()", " ".join(m.group(1).replace("*", " * ").split()), m.group(3).strip()
        if restype not in _RESTYPES:
            raise SehipError("%s: unsupported return type %r" % (where, restype))
        params = [_param(d, where) for d in decls.split(",") if decls not in ("", "void")]
        stream = bool(params) and params[-1].ctype == "se_stream_t"
        prototypes[m.group(2)] = Prototype(restype, tuple(params[:-1] if stream else params), stream)
    return prototypes, defines


with open(HEADER_PATH) as _f:
    PROTOTYPES, DEFINES = parse_header(_f.read())

SE_OK = DEFINES["SE_OK"]
DTYPE_F32, DTYPE_BF16 = DEFINES["SE_DTYPE_F32"], DEFINES["SE_DTYPE_BF16"]
METRIC_COSINE, METRIC_EUCLID, METRIC_DOT = DEFINES["SE_METRIC_COSINE"], DEFINES["SE_METRIC_EUCLID"], DEFINES["SE_METRIC_DOT"]
SVM_GRAD, SVM_HV, SVM_SCORE = DEFINES["SE_SVM_GRAD"], DEFINES["SE_SVM_HV"], DEFINES["SE_SVM_SCORE"]
TOPK_MAX = DEFINES["SE_TOPK_MAX"]
# what call() needs of every entry point: the number of arguments a caller passes, (index, tensor dtypes taken) of every pointer
# parameter among them, whether a stream follows, whether it returns a status
_CALLS = {name: (len(p.params), tuple((i, _POINTEES[q.pointee]) for i, q in enumerate(p.params) if q.pointee), p.stream,
                 p.restype == "int") for name, p in PROTOTYPES.items()}
EXPORTS = tuple(sorted(PROTOTYPES))     # every symbol include/sehip.h declares (checked by tests/test_abi.py)


def build(force=False, verbose=False):
    """Compile csrc/*.hip for gfx950 into sehip/libsehip.so (cross-compiles without a GPU)."""
    srcs = [os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith((".hip", ".h"))] + [HEADER_PATH]
    built = [os.path.join(_HERE, "libsehip.so"), TUNING_LIB_PATH]
    stale = any((not os.path.exists(b)) or any(os.path.getmtime(s) > os.path.getmtime(b) for s in srcs if os.path.exists(s))
                for b in built)
    if force or stale:
        cmd = ["make", "-C", _CSRC, "-j8"] + (["-B"] if force else [])
        out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if verbose or out.returncode != 0:
            print(out.stdout)
        if out.returncode != 0:
            raise SehipError("building libsehip.so failed (see output above)")
    return LIB_PATH


_lib = None


def lib():
    """Load libsehip.so (after torch, so both share one HIP runtime) and declare every entry point from include/sehip.h."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SehipError(
            "libsehip.so not found at %s -- run `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C semantic-embeddings_amd/csrc`. There is no CPU fallback." % LIB_PATH)
    L = ctypes.CDLL(LIB_PATH)
    for name, proto in PROTOTYPES.items():
        fn = getattr(L, name)  # AttributeError here means the .so is stale w.r.t. include/sehip.h
        fn.restype = _RESTYPES[proto.restype]
        fn.argtypes = [_SCALARS.get(p.ctype, ctypes.c_void_p) for p in proto.params] + [ctypes.c_void_p] * proto.stream
    _lib = L
    return L


def call(name, *args):
    """Call entry point ``name`` with every argument but the trailing stream, which is the current torch stream.

    A tensor passes its data pointer once its dtype fits the element type of its pointer parameter; None (NULL) and anything else
    pass as they are, to the conversions of the declared ctypes types.  A negative SE_ERR_* code of an ``int`` entry point raises
    ``SehipError``; any other result is returned."""
    nargs, pointers, stream, status = _CALLS[name]
    if len(args) != nargs:
        raise SehipError("%s takes %d arguments before the stream, got %d" % (name, nargs, len(args)))
    argv = list(args)
    for i, dtypes in pointers:
        a = args[i]
        if isinstance(a, torch.Tensor):
            if a.dtype not in dtypes:
                p = PROTOTYPES[name].params[i]
                raise SehipError("%s: parameter %d (%s %s) cannot take a %s tensor" % (name, i, p.ctype, p.name, a.dtype))
            argv[i] = a.data_ptr()
    if stream:
        argv.append(stream_ptr())
    rc = getattr(lib(), name)(*argv)
    if status and rc < 0:
        check(rc, name)
    return rc


def check(rc, what):
    if rc != SE_OK:
        msg = lib().se_last_error()
        raise SehipError("%s failed (code %d): %s" % (what, rc, msg.decode() if msg else ""))


def require_gpu(*tensors):
    """The product path refuses to run anywhere but on a ROCm device."""
    if not torch.cuda.is_available():
        raise SehipError("sehip kernels need a ROCm GPU (torch.cuda.is_available() is False); "
                         "there is no CPU fallback")
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise SehipError("sehip kernels take device tensors; got a %s tensor" % t.device)


def stream_ptr():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)
