"""The parser of the public headers under include/ that the host-side ABI tests (tests/test_*_host.py) share: a header's wf_* prototypes and
struct fields as argument classes, and the class of a ctypes type, so that a module's PROTOTYPES table and its ctypes structures can be held
against the header position by position.  A plain helper module, as tests/sampler_law.py is."""
import ctypes
import re

SCALAR = {"int": "i32", "int32_t": "i32", "int64_t": "i64", "uint64_t": "u64", "float": "f32", "double": "f64"}


def no_comments(header):
    """The text of the header at this path without its /* ... */ comments."""
    return re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)


def c_class(text, is_return=False):
    """The class of a C type as written ("const float*", "int64_t"): pointer, i32, i64, u64, f32, f64; for a return type also string and void."""
    words = [w for w in text.replace("*", " * ").split() if w != "const"]
    if "*" in words:
        return "string" if is_return and words[0] == "char" else "pointer"
    if is_return and words == ["void"]:
        return "void"
    return SCALAR[words[0]]   # KeyError: a type these tests do not know


def header_prototypes(header):
    """name -> (class of the return type, [class per argument]) for every wf_* function the header declares, in its order."""
    out = {}
    for ret, name, args in re.findall(r"^([\w \*]+?)\b(wf_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", no_comments(header), flags=re.M):
        args = [a.strip() for a in args.split(",")]
        assert name not in out, name
        out[name] = (c_class(ret, True), [] if args == ["void"] else [c_class(a.rsplit(None, 1)[0] if "*" not in a else a) for a in args])
    return out


def ctypes_class(t):
    """The class of a ctypes restype / argtype / field type, in the words of c_class."""
    if t is None:
        return "void"
    if isinstance(t, type) and issubclass(t, ctypes._Pointer):
        return "pointer"
    return {ctypes.c_void_p: "pointer", ctypes.c_char_p: "string", ctypes.c_int32: "i32", ctypes.c_int64: "i64", ctypes.c_uint64: "u64",
            ctypes.c_float: "f32", ctypes.c_double: "f64"}[t]
