"""Reads include/transhuman_hip.h: the ctypes prototypes, Structure classes and constants of the binding (hip.py) come from
the header's own text, so an entry point is written down in C only.  The header is regular C89 declarations; anything this
reader does not recognise raises HeaderError with the line -- nothing is skipped."""
import collections
import ctypes as C
import functools
import re

from .build import HEADER

SCALARS = {"int": C.c_int, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t, "long long": C.c_longlong,
           "int32_t": C.c_int32, "uint32_t": C.c_uint32}
RECORD_CODES = {C.c_void_p: "<u8", C.c_float: "<f4", C.c_uint32: "<u4"}
_BASE = r"(?:const\s+)?(unsigned long long|long long|\w+)\b"
_STATEMENT = re.compile(r"\s*([^;{}]*(?:\{[^{}]*\}[^;{}]*)?);")          # up to a `;` outside braces

# prototypes: name -> (restype, [argtypes]); structs: C name -> Structure class; records: C name -> numpy dtype list;
# constants: name -> int
Header = collections.namedtuple("Header", "prototypes structs records constants")


class HeaderError(ValueError):
    pass


def class_name(c_name):
    return "".join(w.capitalize() for w in c_name.split("_"))          # th_map_source -> ThMapSource


def parse(text, records=("th_adam_tensor",), where="header"):
    """`records`: structs that are filled column-wise through numpy and handed over as a plain address: they become dtype
    lists instead of classes, and a pointer to one stays c_void_p."""
    out = Header({}, {}, {}, {})
    handles = set()                                                    # typedef void* NAME: passed by value as c_void_p

    def fail(pos, what):
        raise HeaderError(f"{where}:{body.count(chr(10), 0, pos) + 1}: cannot parse {' '.join(what.split())!r}")

    def number(s, pos):
        try:
            return int(s.strip().rstrip("uU"), 0)
        except ValueError:
            fail(pos, s)

    def ctype(base, stars, pos, decl):
        if stars:
            if base == "char" and stars == 1:
                return C.c_char_p
            if base in out.structs and stars == 1:
                return C.POINTER(out.structs[base])
            # Every other pointer, device or host, typed or not: ctypes then takes arrays, byref(), pointer instances, ints
            # and None alike -- and no longer refuses a host array of the wrong element type.
            return C.c_void_p
        if base in SCALARS:
            return SCALARS[base]
        if base in handles:
            return C.c_void_p
        if base in out.structs:
            return out.structs[base]
        fail(pos, decl)

    def value_type(decl, pos):
        """`const float* const* name` / `long long` / `void` -> ctypes type (None for void); the name is optional"""
        m = re.fullmatch(_BASE + r"((?:\s*\*|\s*const\b)*)\s*\w*", decl.strip())
        if not m:
            fail(pos, decl)
        stars = m.group(2).count("*")
        return None if (m.group(1), stars) == ("void", 0) else ctype(m.group(1), stars, pos, decl)

    def fields(block, pos):
        res = []
        for decl in filter(None, (d.strip() for d in block.split(";"))):
            m = re.fullmatch(_BASE + r"(.*)", decl, flags=re.S)
            if not m:
                fail(pos, decl)
            for d in m.group(2).split(","):                            # `int R, S` / `const float *p, *q` / `int32_t dims[6]`
                dm = re.fullmatch(r"\s*(\**)\s*(\w+)\s*(?:\[(\d+)\])?\s*", d)
                if not dm:
                    fail(pos, decl)
                t = C.c_void_p if dm.group(1) else ctype(m.group(1), 0, pos, decl)      # (a pointer field is an address)
                res.append((dm.group(2), t * int(dm.group(3)) if dm.group(3) else t))
        return res

    # comments and preprocessor lines leave their line breaks behind, so positions still give the header's line numbers
    body = re.sub(r"/\*.*?\*/", lambda m: " " + "\n" * m.group(0).count("\n"), text, flags=re.S)
    for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(\S.*)$", body, flags=re.M):
        out.constants[m.group(1)] = number(m.group(2), m.start())
    body = re.sub(r"^[ \t]*#.*$", "", body, flags=re.M)
    body, n = re.subn(r'extern\s+"C"\s*\{', "", body)
    if n:
        last = body.rfind("}")
        body = body[:last] + " " + body[last + 1:]

    body, pos = body.rstrip(), 0
    while pos < len(body):
        m = _STATEMENT.match(body, pos)
        if not m:
            at = pos + len(body[pos:]) - len(body[pos:].lstrip())
            fail(at, body[at:at + 80])
        stmt, at, pos = m.group(1).strip(), m.start(1), m.end()
        if (e := re.fullmatch(r"enum\s*\{(.*)\}", stmt, flags=re.S)):
            for item in e.group(1).split(","):
                name, eq, val = item.partition("=")
                if not eq or not re.fullmatch(r"\s*\w+\s*", name):
                    fail(at, item)
                out.constants[name.strip()] = number(val, at)
        elif (s := re.fullmatch(r"typedef\s+struct\s*\w*\s*\{(.*)\}\s*(\w+)", stmt, flags=re.S)):
            name, fl = s.group(2), fields(s.group(1), at)
            if name in records:
                if any(t not in RECORD_CODES for _, t in fl):
                    fail(at, stmt)
                out.records[name] = [(f, RECORD_CODES[t]) for f, t in fl]
            else:
                out.structs[name] = type(class_name(name), (C.Structure,), {"_fields_": fl})
        elif re.fullmatch(r"typedef\s+struct\s+(\w+)\s+\1", stmt):       # an opaque handle: only ever seen behind a pointer
            pass
        elif (t := re.fullmatch(r"typedef\s+void\s*\*\s*(\w+)", stmt)):
            handles.add(t.group(1))
        elif (f := re.fullmatch(r"(.*?)\b(\w+)\s*\((.*)\)", stmt, flags=re.S)) and f.group(1).strip():
            args = [] if f.group(3).strip() == "void" else [value_type(a, at) for a in f.group(3).split(",")]
            if None in args or f.group(2) in out.prototypes:
                fail(at, stmt)
            out.prototypes[f.group(2)] = (value_type(f.group(1), at), args)
        else:
            fail(at, stmt)
    return out


@functools.lru_cache(maxsize=None)
def load():
    """the project's header, read once per process"""
    with open(HEADER) as fh:
        return parse(fh.read(), where=HEADER)
