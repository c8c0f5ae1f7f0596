"""The public header's structs as ctypes Structures: what the *_args tests compare the Python bindings and the numpy
record types with."""
import ctypes as C
import os
import re

from conftest import ROOT

CT = {"unsigned": C.c_uint, "int": C.c_int, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "double": C.c_double,
      "float": C.c_float}


def header_struct(name):
    """The fields of `typedef struct { ... } name;` in the header as a ctypes Structure (arrays as name[n])."""
    hdr = open(os.path.join(ROOT, "include", "fmradion_amd.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\}\s*" + name + r"\s*;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        typ, names = decl.split(None, 1)
        for n in names.split(","):
            m = re.fullmatch(r"(\w+)(?:\[(\d+)\])?", n.strip())
            fields.append((m.group(1), CT[typ] * int(m.group(2)) if m.group(2) else CT[typ]))
    return type(name, (C.Structure,), {"_fields_": fields})
