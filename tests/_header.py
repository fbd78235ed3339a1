"""The tests' own reading of include/evk.h, stated once.  It shares nothing with event_utils_amd._lib._read_header, which reads
the same header for the product: two readers that have to agree are the check."""
import ctypes
import os
import re

PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "evk.h")
TEXT = open(PATH).read()
CODE = re.sub(r"/\*.*?\*/", "", TEXT, flags=re.S)                                  # the header without its comments
CALLBACKS = set(re.findall(r"\btypedef\b[^;]*?\(\s*\*\s*(\w+)\s*\)", CODE))        # the function-pointer typedefs
SCALARS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64,
           "float": ctypes.c_float, "double": ctypes.c_double}
RETURNS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "const char *": ctypes.c_char_p}


def ctype(arg):
    """The ctypes type one parameter of a prototype crosses as: every pointer and callback as void*."""
    arg = " ".join(arg.split())
    if "*" in arg or arg.rsplit(" ", 1)[0] in CALLBACKS:
        return ctypes.c_void_p
    return SCALARS[arg.rsplit(" ", 1)[0]]


def prototypes(prefix="evk_"):
    """{name: ([ctypes of the arguments], ctypes return type)} of the declared entry points whose names start with prefix."""
    found = {}
    for m in re.finditer(r"\b(int|int64_t|const char \*)\s*(%s[a-z0-9_]*)\s*\(([^)]*)\)\s*;" % prefix, CODE):
        args = m.group(3).strip()
        assert m.group(2) not in found, m.group(2)
        found[m.group(2)] = ([] if args == "void" else [ctype(a) for a in args.split(",")], RETURNS[m.group(1)])
    return found


def defines():
    """{name: value} of every `#define EVK_X <integer literal>`: decimal or hex, optionally negative, optionally in one pair of
    parentheses, optionally suffixed u, U, l or ll."""
    literal = r"(-?(?:0[xX][0-9a-fA-F]+|\d+))(?:[uU]|ll?)?"
    return {m.group(1): int(m.group(2) or m.group(3), 0)
            for m in re.finditer(r"^#define\s+(EVK_[A-Z0-9_]+)\s+(?:\(%s\)|%s)\s*$" % (literal, literal), CODE, re.M)}
