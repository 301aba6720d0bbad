"""The text of include/dgn_hip.h -> the ctypes objects of the binding (dgn_amd/_lib.py): constants, structs, prototypes.

``parse`` accepts exactly what that header is made of -- comments, the include guard, the two #include lines, the extern "C" guards,
``#define NAME <int>``, enums with explicit values, ``typedef struct X {...} X;`` and prototypes -- and raises ``ValueError`` on
anything else: text it skipped could be an entry point called on ctypes' defaults or a struct with a field missing.
"""
from __future__ import annotations

import ctypes as C
import re
from typing import NamedTuple

_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "size_t": C.c_size_t,
            "float": C.c_float, "double": C.c_double}
_POINTEES = {"void", "char", "unsigned char", *_SCALARS}      # what a pointer may point to, besides the header's structs

_ITEM = re.compile(r"""\s*(?:
      \#ifndef\s+(?P<guard>\w+)\s*\n\s*\#define\s+(?P=guard)[ \t]*\n          # include guard ...
    | \#endif[ \t]*\n                                                       # ... and its end
    | \#include\s*<std(?:def|int)\.h>[ \t]*\n
    | \#ifdef\s+__cplusplus\s*\n\s*(?:extern\s+"C"\s*\{|\})\s*\n\s*\#endif[ \t]*\n
    | \#define\s+(?P<define>\w+)[ \t]+(?P<value>-?\d+)[ \t]*\n
    | enum\s*\{(?P<enum>[^{}]*)\}\s*;
    | typedef\s+struct\s+(?P<struct>\w+)\s*\{(?P<fields>[^{}]*)\}\s*(?P=struct)\s*;
    | (?P<ret>[\w\s*]+?)\b(?P<func>\w+)\s*\((?P<params>[^()]*)\)\s*;
    )""", re.X)
_DECLARATOR = re.compile(r"(.+?)\b(\w+)(?:\[(\w+)\])?$", re.S)      # type, name, array length


class Header(NamedTuple):
    constants: dict       # #defines and enumerators: name -> int
    structs: dict         # name -> ctypes.Structure subclass
    prototypes: dict      # function -> (restype, [argtypes]), in header order


def _ctype(spec: str, structs: dict):
    """One rule for fields, arguments and results: scalars by width, ``Struct*`` typed, ``char*`` a C string, ``T**`` an array of
    addresses, every other pointer an address."""
    words = spec.replace("*", " * ").split()
    stars, base = words.count("*"), " ".join(w for w in words if w not in ("const", "*"))
    if stars == 0 and base in _SCALARS:
        return _SCALARS[base]
    if stars == 1 and base in structs:
        return C.POINTER(structs[base])
    if stars == 1 and base in _POINTEES:
        return C.c_char_p if base == "char" else C.c_void_p
    if stars == 2 and base in _POINTEES:
        return C.POINTER(C.c_void_p)
    raise ValueError(f"dgn_hip.h: unknown type '{spec.strip()}'")


def _declarator(text: str):
    m = _DECLARATOR.match(text.strip())
    if m is None:
        raise ValueError(f"dgn_hip.h: cannot parse the declarator '{text.strip()}'")
    return m.groups()


def _fields(body: str, constants: dict, structs: dict) -> list:
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        first, *more = decl.split(",")                      # int32_t n_towers, f_in, f_out;
        spec, *declared = _declarator(first)
        more = [re.fullmatch(r"\s*(\w+)(?:\[(\w+)\])?\s*", m) for m in more]
        if more and ("*" in spec or None in more):
            raise ValueError(f"dgn_hip.h: only plain names may share a type: '{decl}'")
        for name, dim in [declared] + [m.groups() for m in more]:
            ctype = _ctype(spec, structs)
            if dim is not None:
                if not dim.isdigit() and dim not in constants:
                    raise ValueError(f"dgn_hip.h: unknown array length in '{decl}'")
                ctype = ctype * (int(dim) if dim.isdigit() else constants[dim])
            fields.append((name, ctype))
    return fields


def parse(text: str) -> Header:
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S) + "\n"
    h = Header({}, {}, {})
    pos, end = 0, len(text.rstrip())
    while pos < end:
        m = _ITEM.match(text, pos)
        if m is None:
            raise ValueError(f"dgn_hip.h: cannot classify the text at '{text[pos:pos + 80].strip()}'")
        pos = m.end()
        if m["define"]:
            h.constants[m["define"]] = int(m["value"])
        elif m["enum"] is not None:
            for item in m["enum"].split(","):
                e = re.fullmatch(r"\s*(\w+)\s*=\s*(-?\d+)\s*", item)
                if e is None:
                    raise ValueError(f"dgn_hip.h: enumerator without an explicit value: '{item.strip()}'")
                h.constants[e[1]] = int(e[2])
        elif m["struct"]:
            h.structs[m["struct"]] = type(m["struct"], (C.Structure,), {"_fields_": _fields(m["fields"], h.constants, h.structs)})
        elif m["func"]:
            params = [] if m["params"].strip() == "void" else [_declarator(p) for p in m["params"].split(",")]
            if any(dim is not None for _, _, dim in params):
                raise ValueError(f"dgn_hip.h: array parameter of {m['func']}")
            h.prototypes[m["func"]] = (_ctype(m["ret"], h.structs), [_ctype(spec, h.structs) for spec, _, _ in params])
    return h
