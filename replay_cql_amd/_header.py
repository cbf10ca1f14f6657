"""Reader of include/cqlrec.h: the constants, the phase enum, the structs and the prototypes as ctypes objects, so that
`_native` restates none of them.  Pure Python, no torch, no library load.

It knows what that header uses and nothing else -- comments, `#define CQLREC_NAME <integer>`, one anonymous enum,
`typedef void* cqlrec_stream`, `typedef struct`s of scalar / pointer / nested-struct fields, prototypes -- and raises
CqlrecError, naming the text, on anything it does not recognise: there is no fallback table.

Types: scalars by `_SCALARS`; a returned `const char*` -> c_char_p; a pointer to a cqlrec_* struct -> POINTER of its
Structure; a pointer parameter whose own text carries a `[host]` comment -> POINTER of the pointee's scalar; every other
pointer, and cqlrec_stream, -> `vp` (a device pointer: `_device.Engine` passes a tensor's data_ptr() there)."""
from __future__ import annotations

import ctypes as C
import re
from pathlib import Path
from types import SimpleNamespace

HEADER = Path(__file__).resolve().parent.parent / "include" / "cqlrec.h"
vp, i32, i64, u32, u64, f32, f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32, C.c_uint64, C.c_float, C.c_double
_SCALARS = {"int": i32, "int32_t": i32, "int64_t": i64, "uint32_t": u32, "uint64_t": u64, "float": f32, "double": f64,
            "uint8_t": C.c_uint8, "uint16_t": C.c_uint16}
_GUARDS = ("#ifndef CQLREC_H", "#define CQLREC_H", "#include <stdint.h>", "#endif")
_HOST = "@host"                                                  # what a comment that holds [host] is replaced by
_DEFINE = re.compile(r"#define CQLREC_(\w+) (\(-?\d+\)|-?\d+)")
_SKIP = re.compile(rf"(\s|{_HOST})*")                            # between declarations a marker says nothing
_DECL = re.compile(r"typedef\s+void\s*\*\s*cqlrec_stream\s*;"
                   r"|typedef\s+struct\s+\w+\s*\{(?P<body>[^{}]*)\}\s*(?P<struct>\w+)\s*;"
                   r"|enum\s*\{(?P<enum>[^{}]*)\}\s*;"
                   r"|(?P<ret>const\s+char\s*\*|\w+)\s*(?P<fn>cqlrec_\w+)\s*\((?P<params>[^(){};]*)\)\s*;")
_VAR = re.compile(r"(?:const\s+)?(\w+)\s*(\*?)\s*(\w+)")


class CqlrecError(RuntimeError):
    pass


def _camel(name: str) -> str:
    return "".join(w.title() for w in name[len("cqlrec_"):].split("_"))


def parse(text: str, mixins=None):
    """constants {NAME: int} and enum {NAME: int} without the CQLREC_ prefix, structs {PyName: Structure}
    (cqlrec_train_ctx is TrainCtx; `mixins` {PyName: class} adds methods), signatures {symbol: (restype, [argtypes])}"""
    text = re.sub(r"/\*.*?\*/", lambda m: f" {_HOST} " if "[host]" in m.group(0) else " ", text, flags=re.S)
    text = re.sub(r"#ifdef __cplusplus\n(extern \"C\" \{|\})\n#endif", "", text)
    const, enum, structs, sigs, decls = {}, {}, {}, {}, []
    for line in text.splitlines():
        if not line.startswith("#"):
            decls.append(line)
            continue
        line = line.replace(_HOST, "").strip()
        m = _DEFINE.fullmatch(line)
        if m:
            const[m.group(1)] = int(m.group(2).strip("()"))
        elif line not in _GUARDS:
            raise CqlrecError(f"cqlrec.h: directive not recognised: {line}")
    text = "\n".join(decls)

    def ctype(base, ptr, host, what):
        """the ctypes type of `base` (ptr: `base*`) in the declaration `what`"""
        if base not in _SCALARS and base not in structs and not (ptr and base == "void") or (host and not ptr):
            raise CqlrecError(f"cqlrec.h: type not recognised in `{what}`")
        if not ptr:
            return _SCALARS.get(base) or structs[base]
        if base in structs and host is not None:                 # host None: a struct's field, where a pointer is a vp
            return C.POINTER(structs[base])
        if host and base not in _SCALARS:
            raise CqlrecError(f"cqlrec.h: [host] pointer to no scalar in `{what}`")
        return C.POINTER(_SCALARS[base]) if host else vp

    def fields(body):
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            first, *more = decl.split(",")                       # `int32_t *users, *tpos`: the base type stands once
            m = _VAR.fullmatch(first.strip())
            rest = [re.fullmatch(r"\s*(\*?)\s*(\w+)\s*", d) for d in more]
            if not m or not all(rest):
                raise CqlrecError(f"cqlrec.h: field not recognised: `{decl}`")
            for ptr, name in [m.group(2, 3)] + [r.group(1, 2) for r in rest]:
                yield name, ctype(m.group(1), ptr, None, decl)

    def param(p, proto):
        m = _VAR.fullmatch(p.replace(_HOST, "").strip())
        if not m:
            raise CqlrecError(f"cqlrec.h: parameter `{p.strip()}` of `{proto}` not recognised")
        return vp if m.group(1, 2) == ("cqlrec_stream", "") else ctype(m.group(1), m.group(2), _HOST in p, p.strip())

    pos = _SKIP.match(text).end()
    while pos < len(text):
        m = _DECL.match(text, pos)
        if not m or (m.group("enum") is not None and enum):
            what = " ".join(text[pos:text.find(";", pos) + 1].split())
            raise CqlrecError(f"cqlrec.h: declaration not recognised: {what}")
        if m.group("struct"):
            py = _camel(m.group("struct"))
            bases = tuple(filter(None, [(mixins or {}).get(py)])) + (C.Structure,)
            structs[m.group("struct")] = type(py, bases, {"_fields_": list(fields(m.group("body")))})
        elif m.group("enum") is not None:
            nxt = 0
            for e in filter(None, (e.strip() for e in m.group("enum").split(","))):
                k = re.fullmatch(r"CQLREC_(\w+?)(?:\s*=\s*(-?\d+))?", e)
                if not k:
                    raise CqlrecError(f"cqlrec.h: enumerator not recognised: `{e}`")
                enum[k.group(1)] = nxt = int(k.group(2)) if k.group(2) else nxt
                nxt += 1
        elif m.group("fn"):
            proto, ret, params = " ".join(m.group(0).split()), m.group("ret"), m.group("params").strip()
            res = C.c_char_p if "char" in ret else vp if ret == "cqlrec_stream" else ctype(ret, "", False, proto)
            sigs[m.group("fn")] = (res, [] if params == "void" else [param(p, proto) for p in params.split(",")])
        pos = _SKIP.match(text, m.end()).end()
    named = len(re.findall(r"\bcqlrec_[a-z0-9_]+\s*\(", re.sub(r"\{[^{}]*\}", "", text)))
    if len(sigs) != named:
        raise CqlrecError(f"cqlrec.h: {len(sigs)} prototypes read, cqlrec_*( stands {named} times outside the structs")
    structs = {_camel(n): s for n, s in structs.items()}
    return SimpleNamespace(constants=const, enum=enum, structs=structs, signatures=sigs)


def read(path: Path = HEADER, mixins=None):
    if not Path(path).exists():
        raise CqlrecError(f"{path} is missing: the ctypes binding is read from it, and there is no fallback table")
    return parse(Path(path).read_text(encoding="utf-8"), mixins)
