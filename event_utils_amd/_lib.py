"""ctypes binding of libevk.so, derived from include/evk.h: the header's #define EVK_* constants become this module's
attributes and its prototypes become PROTOTYPES.  There is NO fallback: if the HIP library is missing or cannot be
loaded the product fails loudly -- build it with `python -m event_utils_amd.csrc.build` (or __graft_entry__.build())."""
import ctypes
import os
import re
from ctypes import c_char_p, c_double, c_float, c_int, c_int64, c_uint32, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
_ENV_DATA = getattr(os.environ, "_data", None)     # posix: {bytes: bytes}, the dict behind os.environ (kept in step by setenv / monkeypatch)
_ENV_KEYS = {}


def getenv(name, default):
    """os.environ.get(name, default) without its per-call encode / decode machinery (~0.7 us each, seven of them on the
    path of one public call: with synchronous error reports the host's share of a call is on the critical path)."""
    if _ENV_DATA is None or type(_ENV_DATA) is not dict:
        return os.environ.get(name, default)
    k = _ENV_KEYS.get(name)
    if k is None:
        k = _ENV_KEYS[name] = os.fsencode(name)
    v = _ENV_DATA.get(k)
    return default if v is None else os.fsdecode(v)


LIB_PATH = os.environ.get("EVK_LIB_PATH") or os.path.join(_HERE, "csrc", "libevk.so")   # EVK_LIB_PATH: A/B builds
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "evk.h")


class EvkError(RuntimeError):
    pass


_SCALARS = {"int": c_int, "int64_t": c_int64, "uint32_t": c_uint32, "uint64_t": c_uint64, "float": c_float, "double": c_double}
_RETURNS = {"int": c_int, "int64_t": c_int64, "const char *": c_char_p}
_DEFINE = re.compile(r"^#define[ \t]+(EVK_[A-Z0-9_]+)[ \t]*(.*)$", re.M)
_LITERAL = re.compile(r"(\()?(-?(?:0[xX][0-9a-fA-F]+|0|[1-9][0-9]*))(?:[uU]|ll?)?(?(1)\))")
_TYPEDEF = re.compile(r"^typedef\b[^;]*;", re.M)
_PROTOTYPE = re.compile(r"^([A-Za-z_][\w \t*]*?)\b(evk_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", re.M)


def _read_header(text):
    """(constants, prototypes) of a header in the style include/evk.h states: {EVK_X: int} and {evk_x: (argtypes, restype)},
    every pointer void*.  Anything it cannot read raises EvkError: a declaration must never silently lose its binding."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    constants, prototypes, callbacks = {}, {}, set()
    for name, value in _DEFINE.findall(text):
        m = _LITERAL.fullmatch(value.strip())
        if name in constants:
            raise EvkError("evk.h: %s is defined twice" % name)
        if m:
            constants[name] = int(m.group(2), 0)
        elif value.strip():                                           # the include guard has no value
            raise EvkError("evk.h: #define %s %s is not an integer literal" % (name, value.strip()))

    def typedef(m):
        callbacks.update(re.findall(r"\(\s*\*\s*(\w+)\s*\)", m.group(0)))
        return ""

    def prototype(m):
        ret, name = " ".join(m.group(1).replace("*", " * ").split()), m.group(2)
        params = [" ".join(a.split()) for a in m.group(3).split(",")]
        if ret not in _RETURNS:
            raise EvkError("evk.h: %s: unknown return type '%s'" % (name, ret))
        if name in prototypes:
            raise EvkError("evk.h: %s is declared twice" % name)
        argtypes = []
        for a in params if params != ["void"] else []:
            kind = a.rsplit(" ", 1)[0]
            if "*" in a or kind in callbacks:
                argtypes.append(c_void_p)
            elif kind in _SCALARS:
                argtypes.append(_SCALARS[kind])
            else:
                raise EvkError("evk.h: %s: unknown parameter type '%s'" % (name, a))
        prototypes[name] = (argtypes, _RETURNS[ret])
        return ""

    rest = _PROTOTYPE.sub(prototype, _TYPEDEF.sub(typedef, text))
    stray = re.search(r"\b(evk_[a-z0-9_]+)\s*\(", rest)
    if stray:
        raise EvkError("evk.h: cannot read the declaration of %s" % stray.group(1))
    return constants, prototypes


def _load_header():
    try:
        with open(HEADER_PATH) as f:
            return _read_header(f.read())
    except OSError as e:
        raise EvkError("cannot read the C header %s (%s): the binding is derived from it" % (HEADER_PATH, e))


_CONSTANTS, PROTOTYPES = _load_header()     # read once, at import; nothing on a call path reads the header again
globals().update(_CONSTANTS)                # EVK_* as plain ints

_lib = None


def lib():
    """The loaded library (loads on first use; raises if it is not built -- never falls back to a CPU path)."""
    global _lib
    if _lib is None:
        if not os.path.isfile(LIB_PATH):
            raise EvkError("libevk.so is not built (%s missing): run `python -m event_utils_amd.csrc.build`; "
                           "event_utils_amd has no CPU fallback" % LIB_PATH)
        try:
            L = ctypes.CDLL(LIB_PATH)
        except OSError as e:
            raise EvkError("cannot load %s: %s" % (LIB_PATH, e))
        for name, (argtypes, restype) in PROTOTYPES.items():
            fn = getattr(L, name)
            fn.argtypes = argtypes
            fn.restype = restype
        _lib = L
    return _lib


def check(rc, what=""):
    if rc != 0:
        msg = lib().evk_error_string(rc)
        raise EvkError("%s failed: %s (code %d)" % (what or "evk call", msg.decode() if msg else "?", rc))


def call(name, *args):
    check(getattr(lib(), name)(*args), name)
