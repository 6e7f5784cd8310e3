"""The C ABI of libgims_hip.so as ctypes, read from include/gims_hip.h: the header is the one place an entry point, a struct or a constant is
written down.  A regex parser of exactly the C the header uses -- `#define GIMS_X <int expr>`, `typedef struct x {...} x;` (members `type a, b;`,
pointers, arrays dimensioned by defines, structs by value, one level of `union {...} u;`) and `ret gims_x(args);` -- that raises on anything
else.  tests/test_host_cpu.py checks what it builds against the C compiler: every size, every offset, every prototype."""
from __future__ import annotations

import ctypes as C
import os
import re
from collections import namedtuple

HEADER_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "gims_hip.h")

SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint8_t": C.c_uint8, "uint16_t": C.c_uint16, "uint32_t": C.c_uint32,
           "uint64_t": C.c_uint64, "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double}

# constants: {"GIMS_X": int}; structs: {"gims_x": ctypes class}, in declaration order; signatures: {"gims_x": (restype, [argtypes])};
# c_types: {"gims_x": (C text of the return type, [C text of every argument type])}
Abi = namedtuple("Abi", "constants structs signatures c_types")


class GimsHipError(RuntimeError):
    pass


_DECL = re.compile(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*\1\s*;"               # 1, 2: typedef struct x { body } x;
                   r"|([\w\s*]+?)\b(gims_\w+)\s*\(([^(){};]*)\)\s*;", re.S)       # 3, 4, 5: ret gims_x(args);
_MEMBER = re.compile(r"((?:const\s+)?(?:struct\s+)?\w+)\b(.*)", re.S)            # type, declarators
_DECLARATOR = re.compile(r"([\s*]*)(\w+)\s*((?:\[[^\]]+\]\s*)*)")                 # stars, name, [dims]
_INT_EXPR = re.compile(r"[\w\s()+\-*|<]+")
_SPACE = re.compile(r"\s*")


def parse(header_path: str = HEADER_PATH) -> Abi:
    if not os.path.exists(header_path):
        raise GimsHipError(f"{header_path} is missing: the ctypes binding is derived from it")
    with open(header_path) as f:
        return parse_text(f.read())


def parse_text(text: str) -> Abi:
    abi = Abi({}, {}, {}, {})

    def fail(what, where):
        raise GimsHipError(f"gims_hip.h, line {text.count(chr(10), 0, where) + 1}: {what}")

    def integer(expr, where):
        if not _INT_EXPR.fullmatch(expr):
            fail(f"not an integer expression: {expr!r}", where)
        try:
            return int(eval(expr, {"__builtins__": {}}, abi.constants))
        except Exception:
            fail(f"cannot evaluate {expr!r}", where)

    def ctype(c_text, where, ret=False):
        base = re.sub(r"\b(const|struct)\b|\*", " ", c_text).strip()
        if "*" in c_text:
            if base not in SCALARS and base not in abi.structs and base not in ("void", "char"):
                fail(f"pointer to unknown type {c_text!r}", where)
            return C.c_char_p if ret and base == "char" else C.c_void_p
        if base not in SCALARS and base not in abi.structs:
            fail(f"unknown type {c_text!r}", where)
        return SCALARS.get(base) or abi.structs[base]

    def fields(owner, body, where):
        out, end = [], 0
        for mm in re.finditer(r"\s*([^;{]*(?:\{.*\}[^;]*)?);", body, re.S):         # one member; the ';' inside a nested { } do not end it
            member, at, end = mm[1].strip(), where + mm.start(1), mm.end()
            u = re.fullmatch(r"union\s*\{(.*)\}\s*(\w+)", member, re.S)
            if u:
                inner = fields(f"{owner}.{u[2]}", u[1], at + mm[1].index("{") + 1)
                out.append((u[2], type(f"{owner}_{u[2]}", (C.Union,), {"_fields_": inner})))
                continue
            m = _MEMBER.fullmatch(member)
            for decl in (m[2].split(",") if m else [""]):
                d = _DECLARATOR.fullmatch(decl.strip())
                if not d:
                    fail(f"cannot parse the member {member!r} of {owner}", at)
                t = ctype(m[1] + d[1].replace(" ", ""), at)
                for dim in reversed(re.findall(r"\[([^\]]+)\]", d[3])):
                    t = t * integer(dim, at)
                out.append((d[2], t))
        if body[end:].strip():
            fail(f"cannot parse the member {body[end:].strip()!r} of {owner} (a missing ';'?)", where + end)
        return out

    # comments and preprocessor lines become blanks of the same number of lines, so that errors can name the line
    text = re.sub(r"/\*.*?\*/", lambda m: "\n" * m[0].count("\n") or " ", text, flags=re.S)
    text = re.sub(r"#ifdef __cplusplus.*?#endif", lambda m: "\n" * m[0].count("\n"), text, flags=re.S)
    for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(GIMS_\w+)[ \t]+(\S.*?)[ \t]*$", text, re.M):
        abi.constants[m[1]] = integer(m[2], m.start())
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    pos = _SPACE.match(text).end()
    while pos < len(text):
        m = _DECL.match(text, pos)
        if not m:
            fail(f"cannot parse the declaration {text[pos:].split(chr(10))[0].strip()!r} (unknown form, or a missing ';')", pos)
        if m[1]:
            abi.structs[m[1]] = type(m[1], (C.Structure,), {"_fields_": fields(m[1], m[2], m.start(2))})
        else:
            args = [] if m[5].strip() == "void" else [re.fullmatch(r"(.*?)\s*\b(\w+)", a.strip(), re.S) for a in m[5].split(",")]
            if not all(a and a[1] for a in args):
                fail(f"cannot parse the arguments of {m[4]}: {' '.join(m[5].split())!r}", pos)
            c_args = [" ".join(a[1].split()) for a in args]
            abi.c_types[m[4]] = (" ".join(m[3].split()), c_args)
            abi.signatures[m[4]] = (ctype(m[3], pos, ret=True), [ctype(a, pos) for a in c_args])
        pos = _SPACE.match(text, m.end()).end()
    return abi
