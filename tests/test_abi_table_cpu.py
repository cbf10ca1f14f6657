"""The ctypes table that `_native` derives from include/cqlrec.h (replay_cql_amd/_header.py), checked four ways; no GPU,
no library load.

1. Against tests/golden/abi_table_known_answers.json: the table `_native.py` held typed by hand, recorded by
   `python tests/test_abi_table_cpu.py --record` from the commit BEFORE the table was derived -- return and argument
   type codes of every entry point, the ordered fields of the four structs, every mirrored constant under its header name and
   PHASES.  It is a frozen record of ABI version 2: names that later changes add are simply absent from it.
2. The four structs against the C++ compiler: sizeof and every offsetof.
3. Strictness: a declaration the reader does not know raises, naming it.
4. The `[host]` rule at the two parameters that lacked the marker."""
import ctypes as C
import json
import re
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from replay_cql_amd import _native as N  # noqa: E402

GOLDEN = ROOT / "tests" / "golden" / "abi_table_known_answers.json"
HEADER = ROOT / "include" / "cqlrec.h"
STRUCTS = {"Layout": "cqlrec_layout", "TrainCtx": "cqlrec_train_ctx", "TrainViews": "cqlrec_train_views",
           "FeaturesPop": "cqlrec_features_pop"}
_CODES = {C.c_int32: "i32", C.c_int64: "i64", C.c_uint32: "u32", C.c_uint64: "u64", C.c_float: "f32", C.c_double: "f64",
          C.c_void_p: "vp", C.c_char_p: "str"}


def code(t) -> str:
    """a ctypes type as text: a scalar's code, a Structure's class name, '*' + the pointee for a typed pointer"""
    if t in _CODES:
        return _CODES[t]
    return t.__name__ if issubclass(t, C.Structure) else "*" + code(t._type_)


def table(native) -> dict:
    const = {}
    for k, v in vars(native).items():
        if k.isupper() and not k.startswith("_") and isinstance(v, int):
            const["FEATURES_" + k[5:] if k.startswith("FEAT_") else k] = v       # the hand-written table said FEAT_*
    weightings = getattr(native, "NEIGHBOUR_WEIGHTINGS")
    const.update({"NEIGHBOUR_WEIGHT_" + ("none" if k is None else k).upper(): v for k, v in weightings.items()})
    return {"signatures": {n: [code(r), [code(a) for a in args]] for n, (r, args) in native.SIGNATURES.items()},
            "structs": {s: [[f, code(t)] for f, t in getattr(native, s)._fields_] for s in STRUCTS},
            "constants": const, "phases": list(native.PHASES)}


@pytest.fixture(scope="module")
def golden():
    return json.loads(GOLDEN.read_text())


def test_derived_table_is_the_hand_written_one(golden):
    got = table(N)
    assert len(golden["signatures"]) == 136 and golden["constants"]["ABI_VERSION"] == 2
    for name, want in golden["signatures"].items():
        assert got["signatures"][name] == want, name
    for name, want in golden["structs"].items():
        assert got["structs"][name] == want, name
    for name, want in golden["constants"].items():
        assert got["constants"][name] == want, name
    assert got["phases"] == golden["phases"]
    assert N.vp is C.c_void_p                                       # Engine._plan tests `t is N.vp`
    assert N.NEIGHBOUR_WEIGHTINGS == {None: 0, "tf_idf": 1, "bm25": 2}
    assert len(N.EVAL_EXTRAS) == 4 and all(isinstance(n, str) for n in N.EVAL_EXTRAS)


def test_structs_match_the_compiler(tmp_path):
    """sizeof and every offsetof, from the host compiler that builds the torch shim"""
    lines = []
    for py, c in STRUCTS.items():
        lines.append(f'  printf("{py} sizeof %zu\\n", sizeof({c}));')
        lines += [f'  printf("{py} {f} %zu\\n", offsetof({c}, {f}));' for f, _ in getattr(N, py)._fields_]
    src = tmp_path / "layout.cpp"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "cqlrec.h"\nint main() {\n' + "\n".join(lines) +
                   "\n  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["g++", "-std=c++17", f"-I{HEADER.parent}", str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    want = {tuple(ln.split()[:2]): int(ln.split()[2]) for ln in out.splitlines()}
    got = {}
    for py in STRUCTS:
        cls = getattr(N, py)
        got[(py, "sizeof")] = C.sizeof(cls)
        got.update({(py, f): getattr(cls, f).offset for f, _ in cls._fields_})
    assert got == want and len(want) == 4 + sum(len(getattr(N, py)._fields_) for py in STRUCTS)


def _with(old: str, new: str) -> str:
    text = HEADER.read_text()
    assert text.count(old) == 1, old
    return text.replace(old, new)


@pytest.mark.parametrize("old,new,names", [
    ("int cqlrec_set_concurrency(int32_t on);", "int cqlrec_set_concurrency(int16_t on);", "int16_t on"),
    ("int cqlrec_set_concurrency(int32_t on);", "int cqlrec_set_concurrency(const short* on /* [host] */);", "short"),
    ("int32_t d;\n  int32_t reserved;", "int32_t d;\n  long reserved;", "long reserved"),
    ("int cqlrec_prof_enable(int32_t on);", "int cqlrec_prof_enable(int32_t on, void (*done)(int32_t));",
     "cqlrec_prof_enable"),
    ("#define CQLREC_SEG_ALIGN 64", "#define CQLREC_SEG_ALIGN 64.0", "CQLREC_SEG_ALIGN"),
    ("#define CQLREC_SEG_ALIGN 64", "#define CQLREC_SEG_ALIGN (1 << 6)", "CQLREC_SEG_ALIGN"),
    ("int cqlrec_prof_enable(int32_t on);", "enum { CQLREC_SECOND = 1 };\nint cqlrec_prof_enable(int32_t on);",
     "CQLREC_SECOND"),
    ("typedef void* cqlrec_stream;", "typedef void* cqlrec_stream;\ntypedef int32_t cqlrec_flag;", "cqlrec_flag"),
    ("int cqlrec_abi_version(void);", "int cqlrec_abi_version(void);\nstatic int two(void) { return 2; }", "two"),
], ids=["scalar", "host-pointee", "field", "function-pointer", "float-define", "expression-define", "second-enum",
        "typedef", "definition"])
def test_reader_is_strict(old, new, names):
    from replay_cql_amd import _header as H
    with pytest.raises(N.CqlrecError, match=re.escape(names)):
        H.parse(_with(old, new))


def test_reader_reports_a_missing_header(tmp_path):
    from replay_cql_amd import _header as H
    with pytest.raises(N.CqlrecError, match=re.escape(str(tmp_path / "cqlrec.h"))):
        H.read(tmp_path / "cqlrec.h")


def test_prototype_count_is_the_declared_one():
    from test_abi import _declared
    assert sorted(N.SIGNATURES) == _declared() and len(N.SIGNATURES) >= 136


def test_host_marker_decides_typed_pointers():
    p32 = C.POINTER(C.c_int32)
    seen = N.SIGNATURES["cqlrec_topk_seen_form"][1]                  # (ws, n_users, n_cand, d, k, out [host], stream)
    assert seen[5] is p32 and seen[0] is N.vp and seen[6] is N.vp and seen[4] is N.i32
    block = N.SIGNATURES["cqlrec_features_block"][1]                 # ..., fi, colmap [host], n_cols, pops, ...
    assert block[11] is p32 and block[8] is N.vp and block[16] is N.vp and (block[10], block[12]) == (N.i32, N.i32)
    assert block[13] is C.POINTER(N.FeaturesPop)
    # every typed pointer of the table is a [host] parameter or a pointer to one of the four structs; nothing else is
    typed = {(n, i) for n, (_, args) in N.SIGNATURES.items() for i, a in enumerate(args) if code(a).startswith("*")}
    text = re.sub(r"/\*.*?\*/", lambda m: "@" if "[host]" in m.group(0) else "", HEADER.read_text(), flags=re.S)
    marked = set()
    for name, params in re.findall(r"\b(cqlrec_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        marked |= {(name, i) for i, p in enumerate(params.split(",")) if "@" in p or re.search(r"\bcqlrec_\w+\s*\*", p)}
    assert typed == marked and len(typed) >= 21                      # ABI version 2 has 21 of them


if __name__ == "__main__" and "--record" in sys.argv:
    parts = [f' "{k}": ' + (json.dumps(v) if isinstance(v, list) else
                            "{\n" + ",\n".join(f'  "{n}": {json.dumps(x)}' for n, x in v.items()) + "\n }")
             for k, v in table(N).items()]
    GOLDEN.write_text("{\n" + ",\n".join(parts) + "\n}\n")
    print(GOLDEN)
