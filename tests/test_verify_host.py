"""hsflow_verify's host side, no GPU: the ABI of version 0.7 (structure sizes in ctypes and in a C99 translation unit, NULL
handles refused), hsflow_compare_planes_host -- the comparison rule compiled for the host from the header the device kernel
is compiled from -- against an independent NumPy statement of that rule, and the line the drop-in class prints."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

TINY = np.float32(1e-30)
WIDTHS = (1, 3, 5, 63, 64, 65, 257, 600)


def numpy_rule(a, b):
    """The rule of include/hsflow.h, section "is it right?", stated over whole arrays."""
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    ab, bb = a.view(np.uint32), b.view(np.uint32)
    differing = ab != bb
    fin_a, fin_b = np.isfinite(a), np.isfinite(b)
    both = fin_a & fin_b
    exempt = differing & both & (np.abs(a) < TINY) & (np.abs(b) < TINY)
    failing = differing & ~exempt
    measured = differing & both
    with np.errstate(all="ignore"):
        absd = np.abs(a - b)                                    # fp32 arithmetic
    def line(bits):
        i = bits.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(2 ** 31) - i, i)
    ulp = np.abs(line(ab) - line(bb))
    idx = np.flatnonzero(failing.ravel())
    return dict(differing=int(differing.sum()), failing=int(failing.sum()), nonfinite=int((~fin_a).sum()),
                first_failing=int(idx[0]) if idx.size else -1,
                max_abs_diff=np.float32(absd[measured].max()) if measured.any() else np.float32(0),
                max_ulp=int(ulp[measured].max()) if measured.any() else 0)


def assert_same(got, want, what):
    g = got.as_dict() if hasattr(got, "as_dict") else got
    for k in ("differing", "failing", "nonfinite", "first_failing", "max_ulp"):
        assert g[k] == want[k], (what, k, g, want)
    assert np.float32(g["max_abs_diff"]).view(np.uint32) == np.float32(want["max_abs_diff"]).view(np.uint32), (what, g, want)


def bits(x):
    return np.array([x], np.uint32).view(np.float32)[0]


def plant(a, b, rng, cases):
    """Writes the (a value, b value) pairs of `cases` at distinct random places of the two planes; returns the places."""
    H, W = a.shape
    places = rng.permutation(H * W)[:len(cases)]
    for p, (x, y) in zip(places, cases):
        a.flat[p], b.flat[p] = x, y
    return places


NAN1, NAN2 = bits(0x7fc00000), bits(0x7fc00001)
PLANTED = [
    (np.float32(0.0), np.float32(-0.0)),                 # differing, 0 apart, exempt
    (NAN1, NAN1),                                        # same bits: not differing, nonfinite
    (NAN1, NAN2),                                        # NaNs of different bits fail
    (NAN1, np.float32(1.5)), (np.float32(1.5), NAN1),    # NaN against a number, either side
    (np.float32(np.inf), np.float32(np.inf)), (np.float32(-np.inf), np.float32(3.0)), (np.float32(2.0), np.float32(np.inf)),
    (np.float32(1e-31), np.float32(2e-31)),              # differing, not failing
    (np.float32(-1e-31), np.float32(2e-31)),             # across zero, still exempt
    (np.float32(1e-31), np.float32(1e-29)),              # failing: one side above the bound
    (np.float32(1e-40), np.float32(3e-40)),              # denormals
    (np.float32(0.7), np.float32(-0.7)),
]


def test_abi_of_version_7(hs):
    L = hs._lib.load()
    PD, VR = hs._lib.HsflowPlaneDiff, hs._lib.HsflowVerifyReport
    assert L.hsflow_version() >= 7
    assert ctypes.sizeof(PD) == 40 and ctypes.sizeof(VR) == 120
    assert VR.u.offset == 24 and VR.v.offset == 64 and VR.deriv_differing.offset == 104 and VR.deriv_first.offset == 112
    assert hs.VERIFY_TINY == 1e-30
    d, r = PD(), VR()
    r.struct_size = ctypes.sizeof(VR)
    buf = (ctypes.c_float * 4)()
    # no device is touched by any of these
    assert L.hsflow_verify(None, 0, ctypes.byref(r)) == hs._lib.E_ARG
    assert L.hsflow_pipeline_verify(None, 0, ctypes.byref(r)) == hs._lib.E_ARG
    assert L.hsflow_compare_flow_device(None, 0, buf, 16, buf, 16, ctypes.byref(d), ctypes.byref(d)) == hs._lib.E_ARG
    assert L.hsflow_compare_planes_host(None, 16, buf, 16, 4, 1, ctypes.byref(d)) == hs._lib.E_ARG
    assert L.hsflow_compare_planes_host(buf, 16, buf, 16, 4, 1, None) == hs._lib.E_ARG
    assert L.hsflow_compare_planes_host(buf, 12, buf, 16, 4, 1, ctypes.byref(d)) == hs._lib.E_SIZE     # stride < 4*width
    assert L.hsflow_compare_planes_host(buf, 18, buf, 16, 4, 1, ctypes.byref(d)) == hs._lib.E_SIZE     # not a multiple of 4
    assert L.hsflow_compare_planes_host(buf, 16, buf, 16, 0, 1, ctypes.byref(d)) == hs._lib.E_SIZE
    assert L.hsflow_last_error(None)
    assert L.hsflow_compare_planes_host(buf, 16, buf, 16, 4, 1, ctypes.byref(d)) == hs._lib.OK
    assert d.differing == 0 and d.first_failing == -1


def test_verify_prototypes_compile_as_c99(hs, tmp_path):
    gcc = shutil.which("gcc")
    if not gcc:
        pytest.skip("no gcc")
    src = tmp_path / "verify.c"
    src.write_text('#include "hsflow.h"\n'
                   "static int (*p0)(const float *, size_t, const float *, size_t, int, int, hsflow_plane_diff *) = hsflow_compare_planes_host;\n"
                   "static int (*p1)(hsflow_ctx *, int, const void *, size_t, const void *, size_t, hsflow_plane_diff *, hsflow_plane_diff *) = hsflow_compare_flow_device;\n"
                   "static int (*p2)(hsflow_ctx *, int, hsflow_verify_report *) = hsflow_verify;\n"
                   "static int (*p3)(hsflow_pipeline *, uint64_t, hsflow_verify_report *) = hsflow_pipeline_verify;\n"
                   "int main(void)\n{\n"
                   "    hsflow_plane_diff d;\n    hsflow_verify_report r;\n"
                   "    float a[6] = {0.0f, 1.0f, 2.0f, 3.0f, 4.0f, 5.0f}, b[6] = {0.0f, 1.0f, 2.5f, 3.0f, 4.0f, 1e-31f};\n"
                   "    if (sizeof d != 40 || sizeof r != 120) return 2;\n"
                   "    r.struct_size = sizeof r;\n"
                   "    if (p2(0, 0, &r) != HSFLOW_E_ARG || p3(0, 0, &r) != HSFLOW_E_ARG || p1(0, 0, a, 12, b, 12, &d, &d) != HSFLOW_E_ARG) return 3;\n"
                   "    if (p0(a, 12, b, 12, 3, 2, &d) != HSFLOW_OK) return 4;\n"
                   "    if (d.differing != 2 || d.failing != 2 || d.nonfinite != 0 || d.first_failing != 2 || d.max_abs_diff != 5.0f) return 5;\n"
                   "    if (!(HSFLOW_VERIFY_TINY == 1e-30f)) return 6;\n"
                   "    return hsflow_version() >= 7 ? 0 : 7;\n}\n")
    libdir = os.path.dirname(hs._lib.LIB_PATH)
    exe = str(tmp_path / "verify")
    r = subprocess.run([gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe, "-L", libdir,
                        "-lhsflow", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, LD_LIBRARY_PATH=libdir + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)


@pytest.mark.parametrize("W", WIDTHS)
def test_host_twin_equals_the_numpy_rule(hs, W):
    rng = np.random.default_rng(1000 + W)
    H = 1 if W == 600 else 37
    H = max(H, -(-len(PLANTED) // W) + 1)
    for pad_a, pad_b in ((0, 0), (3, 0), (0, 5), (2, 7)):
        big_a = rng.standard_normal((H, W + pad_a)).astype(np.float32)
        big_b = np.full((H, W + pad_b), np.float32(9.0))
        a, b = big_a[:, :W], big_b[:, :W]
        b[...] = a
        # equal planes (whatever the padding holds)
        assert_same(hs.compare_planes(a, b), dict(differing=0, failing=0, nonfinite=0, first_failing=-1, max_abs_diff=0, max_ulp=0), (W, "equal"))
        plant(a, b, rng, PLANTED)
        want = numpy_rule(a, b)
        assert want["differing"] > want["failing"] > 0 and want["nonfinite"] == 5, want
        assert_same(hs.compare_planes(a, b), want, (W, pad_a, pad_b))
        assert_same(hs.compare_planes(b, a), numpy_rule(b, a), (W, pad_a, pad_b, "swapped"))


def test_planted_cases_one_by_one(hs):
    base = np.random.default_rng(5).standard_normal((9, 31)).astype(np.float32)

    def one(x, y, at=(4, 17)):
        a, b = base.copy(), base.copy()
        a[at], b[at] = x, y
        return hs.compare_planes(a, b).as_dict()

    idx = 4 * 31 + 17
    d = one(np.float32(0.0), np.float32(-0.0))
    assert (d["differing"], d["failing"], d["first_failing"], d["max_ulp"], d["max_abs_diff"]) == (1, 0, -1, 0, 0.0), d
    d = one(NAN1, NAN1)
    assert (d["differing"], d["failing"], d["nonfinite"]) == (0, 0, 1), d
    d = one(NAN1, np.float32(2.0))
    assert (d["differing"], d["failing"], d["nonfinite"], d["first_failing"], d["max_ulp"], d["max_abs_diff"]) == (1, 1, 1, idx, 0, 0.0), d
    d = one(np.float32(2.0), NAN1)
    assert (d["differing"], d["failing"], d["nonfinite"]) == (1, 1, 0), d
    d = one(np.float32(np.inf), np.float32(np.inf))
    assert (d["differing"], d["nonfinite"]) == (0, 1), d
    d = one(np.float32(1e-31), np.float32(2e-31))
    assert (d["differing"], d["failing"]) == (1, 0) and d["max_abs_diff"] == float(np.float32(2e-31) - np.float32(1e-31)), d
    d = one(np.float32(1e-31), np.float32(1e-29))
    assert (d["differing"], d["failing"], d["first_failing"]) == (1, 1, idx), d
    x = np.float32(0.3)
    d = one(x, bits(int(x.view(np.uint32)) ^ 1))                         # a single lowest-bit flip
    assert (d["differing"], d["failing"], d["max_ulp"], d["first_failing"]) == (1, 1, 1, idx), d
    a, b = base.copy(), base.copy()                                      # two failing elements: the lower index
    a[7, 2], a[2, 30] = 5.0, 6.0
    d = hs.compare_planes(a, b).as_dict()
    assert (d["failing"], d["first_failing"]) == (2, 2 * 31 + 30), d
    # Python-side argument checks
    with pytest.raises(ValueError):
        hs.compare_planes(base, base.astype(np.float64))
    with pytest.raises(ValueError):
        hs.compare_planes(base, base[:3])
    # a transposed view has no unit column stride: it is copied, not misread
    assert hs.compare_planes(base.T, base.T.copy()).differing == 0


def test_verify_line(hs, tmp_path):
    """verify_line (csrc/host/verify_line.hpp), compiled with g++ alone, on hand-made reports."""
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "verify_line")
    r = subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "verify_line_main.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    W = 600
    r = subprocess.run([exe, str(W)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout, r.stderr)
    lines = r.stdout.splitlines()
    assert len(lines) == 5, lines
    assert lines[0].startswith("Passed!") and "sweeps 100" in lines[0] and "reference pass 100" in lines[0]
    # u fails at raster index 123 * W + 45
    assert lines[1].startswith("Failed") and "plane u" in lines[1] and "x 45 y 123" in lines[1] and "max_ulp 1" in lines[1], lines[1]
    # only v fails, in pair 2, at 7 * W + 599
    assert lines[2].startswith("Failed") and "plane v" in lines[2] and "pair 2" in lines[2] and "x 599 y 7" in lines[2] and "0.25" in lines[2], lines[2]
    # only derivative words differ
    assert lines[3].startswith("Failed") and "derivatives" in lines[3] and "x 1 y 2" in lines[3], lines[3]
    # the passes stopped on different sweeps
    assert lines[4].startswith("Failed") and "sweeps 37" in lines[4] and "reference pass 41" in lines[4], lines[4]
