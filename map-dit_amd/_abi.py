"""Strict reader of ``include/mapdit.h``: the one place the C ABI is written down, read into tables ``_lib`` binds from.

A reader for THIS header's grammar, not a C parser.  It knows comments, the include guard, ``#include``, ``#ifdef __cplusplus`` /
``extern "C" {``, integer ``#define``s, ``enum {...};``, ``typedef struct {...} name;``, opaque ``typedef struct tag name;`` and
prototypes over the scalar types below.  Any other non-blank text raises ``AbiError`` quoting it: a declaration that cannot be read
stops the import, it never goes quietly unbound.  Pure Python (``re``, ``ctypes``): importing it loads nothing.
"""
from __future__ import annotations

import ctypes as C
import re
from typing import NamedTuple

SCALARS = {"int": C.c_int, "long": C.c_long, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t,
           "uint8_t": C.c_uint8, "uint16_t": C.c_uint16, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "int64_t": C.c_int64}


class AbiError(ValueError):
    pass


class Abi(NamedTuple):
    functions: dict    # name -> (return C type, [(parameter C type, parameter name), ...])
    structs: dict      # typedef name -> [(field name, C type), ...]
    constants: dict    # enumerator or #define name -> int


_INT = r"-?(?:0[xX][0-9a-fA-F]+|[1-9][0-9]*|0)"
_DIRECTIVE = re.compile(r"#\s*(?:ifndef\s+(?P<guard>\w+)|ifdef\s+__cplusplus|endif|include\s*<[\w./]+>|"
                        r"define\s+(?P<name>\w+)(?:\s+(?P<value>%s))?)\s*" % _INT)
_DECL = re.compile(r"\s*(.*?[\s*])(\w+)\s*")            # 'type name'
_ENUMERATOR = re.compile(r"\s*(\w+)\s*(?:=\s*(%s)\s*)?" % _INT)
_STATEMENTS = [(kind, re.compile(r"\s*(?:%s)" % rx)) for kind, rx in (
    ("extern", r'extern\s+"C"\s*\{|\}'),           # the lone brace closes it
    ("opaque", r"typedef\s+struct\s+\w+\s+(\w+)\s*;"),
    ("struct", r"typedef\s+struct\s*\{([^{}]*)\}\s*(\w+)\s*;"),
    ("enum", r"enum\s*\{([^{}]*)\}\s*;"),
    ("proto", r"((?:\w+[\s*]+)+)(\w+)\s*\(([^(){};]*)\)\s*;"),
)]


def _quote(text):
    return " ".join(text.split())[:120]


def parse(text: str) -> Abi:
    functions, structs, constants, pointees, read = {}, {}, {}, {"void", "char", *SCALARS}, {}

    def ctype_of(decl, what, void_ok=False):
        """'const float* const*' -> 'float**'; the base must be a scalar or, behind a pointer, a type declared above."""
        if decl in read:                   # (a header of 1,500 parameters spells some 30 types)
            return read[decl]
        words = [w for w in decl.replace("*", " * ").split() if w != "const"]
        base, stars = [w for w in words if w != "*"], words.count("*")
        ok = len(base) == 1 and words[len(base):] == ["*"] * stars and (base[0] in pointees if stars else base[0] in SCALARS)
        if not ok:
            if void_ok and words == ["void"]:
                return "void"
            raise AbiError(f"mapdit.h: unknown type in {what}: {_quote(decl)!r}")
        read[decl] = base[0] + "*" * stars
        return read[decl]

    def define(table, name, value, where):
        if name in functions or name in structs or name in constants or name in pointees:
            raise AbiError(f"mapdit.h: {name} is declared twice: {_quote(where)!r}")
        table[name] = value

    text = re.sub(r"/\*.*?\*/", lambda m: " " + "\n" * m.group().count("\n"), text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    lines, guard = text.split("\n"), None
    for i, line in enumerate(lines):
        if line.lstrip().startswith("#"):
            m = _DIRECTIVE.fullmatch(line.strip())
            if not m:
                raise AbiError(f"mapdit.h: unknown preprocessor line: {_quote(line)!r}")
            if m["guard"]:
                guard = m["guard"]
            elif m["value"] is not None:
                define(constants, m["name"], int(m["value"], 0), line)
            elif m["name"] and m["name"] != guard:
                raise AbiError(f"mapdit.h: #define without an integer value that is not the include guard: {_quote(line)!r}")
            lines[i] = ""
    text, pos, open_externs = "\n".join(lines).rstrip(), 0, 0
    while pos < len(text):
        for kind, rx in _STATEMENTS:
            m = rx.match(text, pos)
            if m:
                break
        else:
            raise AbiError(f"mapdit.h: text that is no known declaration: {_quote(''.join(text[pos:].partition(';')[:2]))!r}")
        pos = m.end()
        if kind == "extern":
            open_externs += 1 if m.group().endswith("{") else -1
            if open_externs < 0:
                raise AbiError("mapdit.h: a '}' that closes nothing")
        elif kind == "opaque":
            define({}, m.group(1), None, m.group())
            pointees.add(m.group(1))
        elif kind == "enum":
            value = -1
            for item in m.group(1).split(","):
                e = _ENUMERATOR.fullmatch(item)
                if not e:
                    raise AbiError(f"mapdit.h: enumerator that is no NAME or NAME = integer: {_quote(item) or _quote(m.group())!r}")
                value = int(e.group(2), 0) if e.group(2) else value + 1
                define(constants, e.group(1), value, item)
        elif kind == "struct":
            *members, tail = m.group(1).split(";")
            if tail.strip() or not members:
                raise AbiError(f"mapdit.h: struct member without its ';': {_quote(tail or m.group())!r}")
            fields = []
            for member in members:
                first, *more = member.split(",")
                d = _DECL.fullmatch(first)
                if not d or not all(x.strip().isidentifier() for x in more):     # arrays, bit-fields, '*b' declarators
                    raise AbiError(f"mapdit.h: struct member that is no 'type name[, name]': {_quote(member)!r}")
                ctype = ctype_of(d.group(1), "struct member " + _quote(member))
                fields += [(name.strip(), ctype) for name in [d.group(2), *more]]
            if len({n for n, _ in fields}) != len(fields):
                raise AbiError(f"mapdit.h: {m.group(2)} names a field twice")
            define(structs, m.group(2), fields, m.group(2))
            pointees.add(m.group(2))
        elif kind == "proto":
            ret, name, plist = m.groups()
            params = []
            for p in ([] if plist.strip() == "void" else plist.split(",")):
                d = _DECL.fullmatch(p)
                if not d:                                                             # '...', arrays, unnamed parameters
                    raise AbiError(f"mapdit.h: parameter of {name} that is no 'type name': {_quote(p)!r}")
                params.append((ctype_of(d.group(1), f"parameter of {name}"), d.group(2)))
            define(functions, name, (ctype_of(ret, f"return of {name}", void_ok=True), params), m.group())
    if open_externs:
        raise AbiError('mapdit.h: extern "C" { is never closed')
    return Abi(functions, structs, constants)


def ctype(c_type: str):
    """ctypes type of a parameter or struct field.  Every pointer is c_void_p: the C type cannot tell a host pointer from a device
    address, and c_void_p takes what callers pass for either (int, None, byref(x), ctypes arrays and pointers)."""
    if c_type.endswith("*"):
        return C.c_void_p
    if c_type not in SCALARS:
        raise AbiError(f"mapdit.h: no ctypes type for {c_type!r}")
    return SCALARS[c_type]


def restype(c_type: str):
    return None if c_type == "void" else C.c_char_p if c_type == "char*" else ctype(c_type)


def structure(name: str, fields):
    return type(name, (C.Structure,), {"_fields_": [(f, ctype(t)) for f, t in fields]})
