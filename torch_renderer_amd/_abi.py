"""Reads the C ABI out of the text of ``include/mi355r.h``: the enum constants, the structs as
``ctypes.Structure`` classes and every prototype's ``restype`` / ``argtypes``. The header is the one place
where a signature is decided; ``_lib.py`` binds what this reader returns and mirrors nothing by hand.

The reader knows the few C forms the header uses and refuses the rest: a type outside the tables below
raises ``AbiError`` naming the prototype or struct. It never guesses (ctypes' silent default is ``int``).
"""
from __future__ import annotations

import ctypes
import re
from typing import NamedTuple

_MEMBER = {"float": ctypes.c_float, "double": ctypes.c_double, "int32_t": ctypes.c_int32,
           "int64_t": ctypes.c_int64, "uint8_t": ctypes.c_uint8, "size_t": ctypes.c_size_t}
_PARAM = {k: _MEMBER[k] for k in ("float", "double", "int32_t", "int64_t", "size_t")}
_RETURN = {"const char*": ctypes.c_char_p, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64,
           "size_t": ctypes.c_size_t}
# A pointer to any of these is c_void_p, never POINTER(c_int32) and the like: callers pass c_void_p instances
# (_lib.ptr), data_ptr() integers, None and byref(...), and a typed pointer rejects the first two.
_POINTEE = {*_MEMBER, "uint64_t", "void"}
# A pointer to an ABI struct is POINTER(ThatStruct), with this one exception: view records are a device array
# and callers pass tensors' pointers, so mr_view_t* is c_void_p.
_DEVICE_STRUCTS = {"mr_view_t"}

_DECL = re.compile(r"(?:const\s+)?(\w+)\s*(\*?)\s*(\w*)\s*(?:\[(\d+)\])?")


class AbiError(ValueError):
    pass


class Abi(NamedTuple):
    constants: dict  # MR_* name -> int, every enum of the header
    structs: dict  # class name (mr_raster_settings_t -> MrRasterSettings) -> ctypes.Structure subclass
    prototypes: list  # (name, restype, argtypes) in header order


def _struct(typedef: str, body: str):
    fields = []
    for stmt in filter(None, (s.strip() for s in body.split(";"))):
        first, *more = (d.strip() for d in stmt.split(","))  # `float a[3], b[3]`: the type stands once
        m = _DECL.fullmatch(first)
        if not m or not m[3]:
            raise AbiError(f"struct {typedef}: cannot read member '{stmt}'")
        base = m[1]
        for m in [m, *(_DECL.fullmatch(f"{base} {d}") for d in more)]:
            if not m or not m[3] or (base not in _POINTEE if m[2] else base not in _MEMBER):
                raise AbiError(f"struct {typedef}: unknown member type in '{stmt}'")
            ct = ctypes.c_void_p if m[2] else _MEMBER[base]
            fields.append((m[3], ct * int(m[4]) if m[4] else ct))
    name = "".join(p.capitalize() for p in typedef[:-2].split("_"))
    return name, type(name, (ctypes.Structure,), {"_fields_": fields})


def _param(proto: str, decl: str, by_typedef: dict):
    m = _DECL.fullmatch(decl)
    if not m or m[4]:
        raise AbiError(f"{proto}: cannot read parameter '{decl}'")
    base, star = m[1], m[2]
    if star and base in by_typedef:
        return ctypes.c_void_p if base in _DEVICE_STRUCTS else ctypes.POINTER(by_typedef[base])
    if base not in (_POINTEE if star else _PARAM):
        raise AbiError(f"{proto}: unknown parameter type in '{decl}'")
    return ctypes.c_void_p if star else _PARAM[base]


def read_header(text: str) -> Abi:
    # comments first: they hold text such as `mr_project_faces(+_backward)` that looks like a call
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r'^\s*#.*$|extern\s+"C"\s*\{', " ", text, flags=re.M)

    constants = {}

    def enum(m):
        for item in filter(None, (s.strip() for s in m[1].split(","))):
            kv = re.fullmatch(r"(\w+)\s*=\s*(-?\w+)", item)
            try:
                constants[kv[1]] = int(kv[2], 0)
            except (TypeError, ValueError):
                raise AbiError(f"enum: cannot read '{item}'") from None
        return " "

    text = re.sub(r"\benum\s*\{([^}]*)\}\s*;", enum, text)

    structs, by_typedef = {}, {}

    def struct(m):
        name, cls = _struct(m[2], m[1])
        structs[name] = by_typedef[m[2]] = cls
        return " "

    text = re.sub(r"\btypedef\s+struct\s+\w*\s*\{([^}]*)\}\s*(\w+_t)\s*;", struct, text)

    prototypes = []
    *stmts, tail = text.split(";")
    if tail.replace("}", "").strip():  # (the brace closes extern "C")
        raise AbiError(f"cannot read '{tail.strip()[:60]}'")
    for stmt in stmts:
        m = re.fullmatch(r"\s*(.*?)\s*\b(\w+)\s*\((.*)\)\s*", stmt, flags=re.S)
        if not m:
            raise AbiError(f"cannot read '{' '.join(stmt.split())[:60]}'")
        ret, name, params = re.sub(r"\s*\*", "*", " ".join(m[1].split())), m[2], m[3].strip()
        if ret not in _RETURN:
            raise AbiError(f"{name}: unknown return type '{ret}'")
        args = [] if params == "void" else [_param(name, " ".join(p.split()), by_typedef) for p in params.split(",")]
        prototypes.append((name, _RETURN[ret], args))
    return Abi(constants, structs, prototypes)
