"""The C ABI as ctypes, read from ``include/fie.h``: the header is the one statement of every function, struct and constant.

The header is regular enough for regular expressions (no C parser): comments and preprocessor lines are stripped, ``#define FIE_<NAME> <integer>``
is collected, ``typedef struct fie_X { ... } fie_X;`` bodies give the struct fields and ``ret fie_name(args);`` the functions.  A type this module
does not know raises with the declaration's text: a new type in the header is never guessed.
"""
import ctypes
import os
import re

PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fie.h")

_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double}


def _ctype(text, decl, void=False):
    """ctypes type of the C type `text` (const dropped): char* -> c_char_p, any other pointer -> c_void_p, the scalars above."""
    m = re.fullmatch(r"(\w+)((?:\s*\*)*)", " ".join(re.sub(r"\bconst\b", " ", text).split()))
    if m and m.group(2):
        return ctypes.c_char_p if (m.group(1), m.group(2)) == ("char", "*") else ctypes.c_void_p
    if m and void and m.group(1) == "void":
        return None
    if not m or m.group(1) not in _SCALARS:
        raise TypeError(f"include/fie.h: no ctypes rule for the type {text.strip()!r} in: {' '.join(decl.split())}")
    return _SCALARS[m.group(1)]


def _fields(body, decl):
    """[(name, ctype)] of a struct body: `int a, b;`  `int x[8];`  `int y[4][4];`  `float f;`  `const char* s;`"""
    out = []
    for member in filter(None, (m.strip() for m in body.split(";"))):
        m = re.fullmatch(r"(.*?[\s*])(\w+(?:\s*\[\d+\])*(?:\s*,\s*\w+(?:\s*\[\d+\])*)*)", member, re.S)
        if not m:
            raise TypeError(f"include/fie.h: cannot read the member {member!r} of: {' '.join(decl.split())}")
        base = _ctype(m.group(1), member)
        for item in m.group(2).split(","):
            t = base
            for dim in reversed(re.findall(r"\[(\d+)\]", item)):
                t = t * int(dim)
            out.append((re.match(r"\s*(\w+)", item).group(1), t))
    return out


def parse(text):
    """(defines, structs, functions) of a header: {NAME: int} without the FIE_ prefix, {fie_x: [(field, ctype)]},
    {fie_name: (restype, [argtypes])}."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    defines = {n: int(v, 0) for n, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+FIE_(\w+)[ \t]+\(?(-?\w+?)[uUlL]*\)?[ \t]*$", text, flags=re.M)
               if re.fullmatch(r"-?(0[xX][0-9a-fA-F]+|\d+)", v)}
    text = re.sub(r"^[ \t]*#[^\n]*", " ", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{', " ", text)
    structs = {}

    def struct(m):
        if m.group(1) != m.group(3):
            raise TypeError(f"include/fie.h: typedef struct {m.group(1)} names itself {m.group(3)}")
        structs[m.group(1)] = _fields(m.group(2), m.group(0))
        return " "
    text = re.sub(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", struct, text, flags=re.S)
    functions = {}
    for decl in filter(None, (d.strip() for d in text.replace("}", ";").split(";"))):
        if re.fullmatch(r"typedef\s+struct\s+(\w+)\s+\1", decl):          # opaque handle
            continue
        m = re.fullmatch(r"(.*?[\s*])(fie_\w+)\s*\((.*)\)", decl, re.S)
        if not m:
            raise TypeError(f"include/fie.h: cannot read the declaration: {' '.join(decl.split())}")
        args = [] if m.group(3).strip() in ("", "void") else m.group(3).split(",")
        functions[m.group(2)] = (_ctype(m.group(1), decl, void=True),
                                 [_ctype(re.fullmatch(r"(.*?)\w*", a.strip(), re.S).group(1), decl) for a in args])
    return defines, structs, functions


with open(PATH) as _f:
    DEFINES, STRUCTS, FUNCTIONS = parse(_f.read())

