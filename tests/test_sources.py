"""How the library's sources are cut, kept that way without a GPU: every .hip
under csrc is built, every header there compiles on its own and defines no
kernel, and the ctypes binding's argument lists are the C headers'."""
import ctypes as C
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import __graft_entry__ as g

ROOT = Path(__file__).resolve().parents[1]
INCLUDE = ROOT / "include"


def test_every_source_is_built():
    on_disk = sorted(p.name for p in g.CSRC.glob("*.hip"))
    assert on_disk == sorted(g.SOURCES)
    assert len(set(g.SOURCES)) == len(g.SOURCES)


def test_every_header_stands_alone(tmp_path):
    headers = sorted(g.CSRC.glob("*.h"))
    assert headers

    def syntax_only(h):
        tu = tmp_path / (h.stem + "_alone.hip")
        tu.write_text(f'#include "{h.name}"\n')
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++17", "-fsyntax-only", f"-I{INCLUDE}",
                            f"-I{g.CSRC}", str(tu)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        return h.name, r.returncode, r.stdout

    with ThreadPoolExecutor(max_workers=16) as pool:
        for name, rc, out in pool.map(syntax_only, headers):
            assert rc == 0, f"{name} does not compile by itself:\n{out}"
    # a kernel belongs to a .hip: a header that defines one compiles only where it is included
    for h in headers:
        assert "__global__" not in h.read_text(), h.name


SCALARS = {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "float": C.c_float,
           "double": C.c_double, "size_t": C.c_size_t, "int": C.c_int}


def declared(header):
    """{name: [argument type text, ...]} of a header's `int gsm_*(...)` declarations."""
    text = re.sub(r"/\*.*?\*/", "", (INCLUDE / header).read_text(), flags=re.S)
    out = {}
    for name, args in re.findall(r"^\s*int\s+(gsm_\w+)\s*\(([^)]*)\)\s*;", text, re.M):
        args = " ".join(args.split())
        out[name] = [] if args in ("", "void") else [a.strip() for a in args.split(",")]
    return out


def is_pointer(t):
    return t is C.c_void_p or t is C.c_char_p or (isinstance(t, type) and issubclass(t, C._Pointer))


def test_binding_matches_the_headers():
    from gsmarl_amd import _lib
    for header, table in (("gsm.h", _lib.SIGNATURES), ("gsm_optim.h", _lib.OPTIM_SIGNATURES)):
        decls = declared(header)
        assert set(decls) == set(table), header
        for name, c_args in decls.items():
            res, py_args = table[name]
            assert res is C.c_int, name
            assert len(py_args) == len(c_args), f"{name}: {len(py_args)} bound, {len(c_args)} declared"
            for i, (c_arg, py) in enumerate(zip(c_args, py_args)):
                where = f"{name} argument {i} ({c_arg})"
                if "*" in c_arg:
                    assert is_pointer(py), where
                    continue
                words = [w for w in c_arg.split() if w != "const"]
                assert len(words) == 2 and words[0] in SCALARS, where   # type, then the argument's name
                assert py is SCALARS[words[0]], where
