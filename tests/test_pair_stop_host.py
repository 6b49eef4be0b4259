"""CPU checks of the per-pair stop's interface (include/hsflow.h 0.8): hsflow_set_pair_termination,
hsflow_get_pair_result and hsflow_solve_probe_pairs are declared, exported and bound, hsflow_pair_result has the C
struct's layout, and their argument errors are reported without a GPU.  No compute call is made here."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

NEW = ("hsflow_set_pair_termination", "hsflow_get_pair_result", "hsflow_solve_probe_pairs")


def header_text():
    return open(os.path.join(ROOT, "include", "hsflow.h")).read()


def test_the_three_entry_points_are_declared_exported_and_bound(hs):
    text = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    lib = ctypes.CDLL(hs._lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert hasattr(lib, name), name
        assert name in hs._lib.PROTOTYPES, name
        assert hs._lib.PROTOTYPES[name][0] is ctypes.c_int, name
    assert len(hs._lib.PROTOTYPES["hsflow_set_pair_termination"][1]) == 2
    assert len(hs._lib.PROTOTYPES["hsflow_get_pair_result"][1]) == 3
    assert hs._lib.PROTOTYPES["hsflow_solve_probe_pairs"][1] == hs._lib.PROTOTYPES["hsflow_solve_probe"][1]
    assert hs.HsflowPairResult is hs._lib.HsflowPairResult and "HsflowPairResult" in hs.__all__
    for method in ("set_pair_termination", "pair_results", "solve_probe_pairs"):
        assert callable(getattr(hs.HSFlow, method)), method


def test_version_is_at_least_0_8(hs):
    assert hs._lib.load().hsflow_version() >= 8
    m = re.search(r"#define\s+HSFLOW_VERSION_MINOR\s+(\d+)", header_text())
    assert m and int(m.group(1)) >= 8


def test_pair_result_has_the_c_layout(hs, tmp_path):
    """sizeof and every field offset of hsflow_pair_result, as a C compiler sees the header."""
    R = hs._lib.HsflowPairResult
    names = [n for n, _ in R._fields_]
    assert names == ["struct_size", "pair", "status", "iterations_done", "last_eps", "eps_rerun", "sweeps_executed"]
    assert ctypes.sizeof(R) == 32 and R.sweeps_executed.offset == 24 and R.last_eps.offset == 16
    gcc = shutil.which("gcc")
    if not gcc:
        pytest.skip("no gcc")
    src = tmp_path / "layout.c"
    src.write_text('#include "hsflow.h"\n#include <stddef.h>\n#include <stdio.h>\n'
                   "int main(void)\n{\n"
                   '    printf("%d", (int)sizeof(hsflow_pair_result));\n' +
                   "".join('    printf(" %%d", (int)offsetof(hsflow_pair_result, %s));\n' % n for n in names) +
                   '    printf(" %d\\n", HSFLOW_PAIR_STOP_SIMPLE_CHUNK);\n'
                   "    return 0;\n}\n")
    exe = str(tmp_path / "layout")
    r = subprocess.run([gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.split()]
    assert out[0] == ctypes.sizeof(R), out
    assert out[1:-1] == [getattr(R, n).offset for n in names], out
    assert out[-1] == hs._lib.PAIR_STOP_SIMPLE_CHUNK == 32


def test_argument_errors_without_gpu(hs):
    L = hs._lib.load()
    E_ARG = hs._lib.E_ARG
    r = hs._lib.HsflowPairResult()
    r.struct_size = ctypes.sizeof(r)
    assert L.hsflow_set_pair_termination(None, 1) == E_ARG
    assert L.hsflow_set_pair_termination(None, 0) == E_ARG
    assert L.hsflow_get_pair_result(None, 0, ctypes.byref(r)) == E_ARG
    assert b"null context" in L.hsflow_last_error(None)
    assert L.hsflow_get_pair_result(None, 0, None) == E_ARG
    r.struct_size = 4
    assert L.hsflow_get_pair_result(None, -1, ctypes.byref(r)) == E_ARG
    p = hs.make_params(max_iter=3)
    buf = (ctypes.c_float * 3)()
    assert L.hsflow_solve_probe_pairs(None, ctypes.byref(p), buf) == E_ARG
    assert L.hsflow_solve_probe_pairs(None, None, None) == E_ARG
