"""ctypes loader for libdvm_hip.so (C ABI: include/dvm.h).

There is deliberately no CPU fallback: if the shared library is missing, or a
tensor is not on a HIP device, every op raises.  Build with
`python -c "import __graft_entry__ as g; g.build()"` or `make -C dv-matcher_amd/csrc`.
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(_HERE), "csrc")
SO_PATH = os.path.join(CSRC, "libdvm_hip.so")
HEADER = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "dvm.h")

_lib = None


class DvmError(RuntimeError):
    pass


_SCALARS = {"int": ctypes.c_int, "long": ctypes.c_long, "unsigned": ctypes.c_uint, "unsigned int": ctypes.c_uint,
            "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t}
_DECL = re.compile(r"([\w\s*]+?)\b(dvm_\w+)\s*\(([^()]*)\)")


def _ctype(text, param):
    """The ctypes type of a return type, or of a parameter with or without its name, as the header spells it.  Every pointer
    parameter is a c_void_p (device pointers, host tables and byref() objects all pass); a type not listed here raises."""
    if "*" in text:
        if param:
            return ctypes.c_void_p
        if text.split() == ["const", "char", "*"]:
            return ctypes.c_char_p
    else:
        words = [w for w in text.split() if w != "const"]
        for n in (len(words), len(words) - 1) if param else (len(words),):   # the whole text, then without the parameter's name
            if " ".join(words[:n]) in _SCALARS:
                return _SCALARS[" ".join(words[:n])]
    raise DvmError("include/dvm.h: no ctypes type for the %s `%s`" % ("parameter" if param else "return type", " ".join(text.split())))


def parse_header(src):
    """name -> (restype, [argtypes]) of every `ret dvm_name(args);` in the text of a C header.  Comments, preprocessor lines,
    typedefs and structs are skipped; any other statement that is not such a declaration raises."""
    src = re.sub(r"/\*.*?\*/|//[^\n]*", " ", src, flags=re.S)
    src = re.sub(r"^[ \t]*#.*$", "", src, flags=re.M)
    src = re.sub(r'extern\s*"C"\s*\{', "", src)
    src = re.sub(r"\{[^{}]*\}", "", src).replace("}", "")          # struct bodies; the closing brace of extern "C"
    table = {}
    for stmt in src.split(";"):
        stmt = " ".join(stmt.replace("*", " * ").split())
        if not stmt or stmt.split()[0] in ("typedef", "struct"):
            continue
        m = _DECL.fullmatch(stmt)
        if m is None:
            raise DvmError("include/dvm.h: cannot read the declaration `%s`" % stmt)
        ret, name, args = m.groups()
        args = [] if args.strip() in ("", "void") else args.split(",")
        table[name] = (_ctype(ret, False), [_ctype(a, True) for a in args])
    return table


def _header_text():
    try:
        with open(HEADER) as f:
            return f.read()
    except OSError as e:
        raise DvmError("the C ABI's header was not found at %s (%s): the ctypes prototypes are derived from it" % (HEADER, e))


# name -> (restype, [argtypes]): include/dvm.h, read when this module is imported
SIGNATURES = parse_header(_header_text())


def load():
    """Load the shared library (once). Raises DvmError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise DvmError("libdvm_hip.so not found at %s — build it first (make -C %s); there is no CPU fallback"
                       % (SO_PATH, CSRC))
    lib = ctypes.CDLL(SO_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError here == ABI mismatch, let it propagate
        fn.restype = res
        fn.argtypes = args
    if lib.dvm_abi_version() != 1:
        raise DvmError("libdvm_hip.so ABI version %d != 1" % lib.dvm_abi_version())
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().dvm_last_error()
        raise DvmError("%s failed (%d): %s" % (what, rc, msg.decode() if msg else "?"))
