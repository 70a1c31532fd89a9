"""The ctypes side of the C ABI, read from include/hirl4ucav.h and include/hirl4ucav_debug.h themselves: one ctypes.Structure per
`typedef struct Hx…`, (restype, argtypes) per `hx_*` prototype, the integer `#define HX_*` constants.  A new entry point, struct or constant in
the header needs no line here.  Whatever the reader does not understand raises HxError naming the declaration — it never guesses.
"""
import ctypes
import os
import re

INCLUDE_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
HEADERS = ("hirl4ucav.h", "hirl4ucav_debug.h")

_SCALARS = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64,
            "float": ctypes.c_float, "int": ctypes.c_int}
_RETURNS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "void*": ctypes.c_void_p, "const char*": ctypes.c_char_p}

_STRUCT = re.compile(r"typedef\s+struct\s+(Hx\w+)\s*\{(.*?)\}\s*\1\s*;", re.S)
_PROTO = re.compile(r"(?<![\w*])((?:const\s+)?\w+(?:\s*\*)?)\s*\b(hx_[a-z0-9_]+)\s*\(([^()]*)\)\s*;")
_DEFINE = re.compile(r"^[ \t]*#[ \t]*define[ \t]+(HX_\w+)[ \t]+(?:(\d+)|\(-(\d+)\)|\(1u?[ \t]*<<[ \t]*(\d+)\))[ \t]*$", re.M)


class HxError(RuntimeError):
    pass


class Abi:
    """structs: name -> ctypes.Structure class; functions: name -> (restype, argtypes); defines: name -> int"""

    def __init__(self, structs, functions, defines):
        self.structs, self.functions, self.defines = structs, functions, defines


def _ctype(words, structs, where):
    """the ctypes type of a C type (no declarator name): a scalar, a pointer to one of the derived structs, or c_void_p for any other pointer"""
    words = re.sub(r"\s*\*\s*", "*", " ".join(words.split()))
    if "*" in words:
        m = re.fullmatch(r"(?:const )?(Hx\w+)\*", words)
        if m and m.group(1) not in structs:
            raise HxError(f"{where}: `{words}` points at a struct the headers have not declared before it")
        return ctypes.POINTER(structs[m.group(1)]) if m else ctypes.c_void_p
    scalar = _SCALARS.get(words[6:] if words.startswith("const ") else words)
    if scalar is None:
        raise HxError(f"{where}: unknown type `{words}` (known: {', '.join(_SCALARS)}, pointers)")
    return scalar


def _split(decl, where):
    """`<type> <name>` -> (type, name)"""
    m = re.fullmatch(r"(.*[\s*])(\w+)", decl, re.S)
    if not m:
        raise HxError(f"{where}: cannot read `{' '.join(decl.split())}` as a type and a name (arrays, bit-fields and nested structs are not supported)")
    return m.group(1), m.group(2)


def _fields(name, body, structs):
    out = []
    for decl in (d.strip() for d in body.split(";")):
        if not decl:
            continue
        where = f"struct {name}, field `{' '.join(decl.split())}`"
        first, *more = (p.strip() for p in decl.split(","))  # `float gamma, tau, lr_actor`
        words, field = _split(first, where)
        if more and "*" in decl:
            raise HxError(f"{where}: one pointer per declaration")
        ctype = _ctype(words, structs, where)
        for f in (field, *more):
            if not re.fullmatch(r"\w+", f):
                raise HxError(f"{where}: cannot read `{f}` as a field name (arrays, bit-fields and nested structs are not supported)")
            out.append((f, ctype))
    return out


def parse(text):
    """header text -> Abi"""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    defines = {m.group(1): int(m.group(2)) if m.group(2) else -int(m.group(3)) if m.group(3) else 1 << int(m.group(4))
               for m in _DEFINE.finditer(text)}  # function-like macros and every other kind of value are skipped
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    structs = {}
    for m in _STRUCT.finditer(text):
        structs[m.group(1)] = type(m.group(1), (ctypes.Structure,), {"_fields_": _fields(m.group(1), m.group(2), structs)})
    opened = re.findall(r"\bstruct\s+(\w+)", text)
    if sorted(opened) != sorted(structs):
        raise HxError(f"cannot read the struct declaration(s) {sorted(set(opened) ^ set(structs))} up to `}} Name;`")
    text = _STRUCT.sub("", text)
    functions = {}
    for m in _PROTO.finditer(text):
        ret, name, params = re.sub(r"\s*\*", "*", " ".join(m.group(1).split())), m.group(2), m.group(3).strip()
        if ret not in _RETURNS:
            raise HxError(f"{name}: unknown return type `{ret}` (known: {', '.join(_RETURNS)})")
        args = []
        for i, p in enumerate([] if params in ("", "void") else params.split(",")):
            where = f"{name}, argument {i} `{' '.join(p.split())}`"
            args.append(_ctype(_split(p.strip(), where)[0], structs, where))
        functions[name] = (_RETURNS[ret], args)
    named = set(re.findall(r"\b(hx_[a-z0-9_]+)\s*\(", text))
    if named != set(functions):
        raise HxError(f"cannot read the prototype(s) of {sorted(named ^ set(functions))} up to their `;`")
    return Abi(structs, functions, defines)


_abi = None


def abi():
    """the two headers, parsed once per process"""
    global _abi
    if _abi is None:
        paths = [os.path.join(INCLUDE_DIR, h) for h in HEADERS]
        missing = [p for p in paths if not os.path.exists(p)]
        if missing:
            raise HxError(f"{', '.join(missing)} not found: the binding is read from the C headers in {INCLUDE_DIR}, next to the package")
        _abi = parse("\n".join(open(p).read() for p in paths))
    return _abi


def bind(lib):
    """argtypes and restype of every declared function on a loaded CDLL"""
    for name, (restype, argtypes) in abi().functions.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise HxError(f"{lib._name} does not export {name}, which the headers in {INCLUDE_DIR} declare: a stale or foreign library, rebuild it "
                          f"(make -C hirl4ucav_amd/csrc)") from None
        fn.restype, fn.argtypes = restype, argtypes
