"""CPU checks of the sequence entries (ABI 0.14: hsflow_set_sequence_device_ex, hsflow_set_sequence_jpeg_ex,
hsflow_preprocess_sequence_host): they exist and refuse bad arguments without a GPU, and the sequence rule of
csrc/hs_pre_rule.h -- the one walk the kernel k_pre_sequence and the host entry are compiled from -- equals compositions
of the existing frame rule: p_j = hsflow_preprocess_frame_host(format, f_j), and B(p_j) = GRAY8_BLUR of the BYTES of p_j."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NEW = ["hsflow_set_sequence_device_ex", "hsflow_set_sequence_jpeg_ex", "hsflow_preprocess_sequence_host"]
FORMATS = ["gray", "gray_blur", "bgr", "bgr_blur"]
FLAGS = [0, 1, 3]
COUNTS = [2, 3, 5]
SHAPES = [(1, 1), (2, 1), (1, 2), (3, 3), (5, 2), (4, 7), (7, 9), (8, 8), (9, 16), (13, 17), (255, 8), (257, 10)]  # W x H


def header():
    return open(os.path.join(ROOT, "include", "hsflow.h")).read()


def reblurred(flags, k):
    return bool(flags & 1) and (k > 0 or bool(flags & 2))


def composed(hs, frames, fmt, flags):
    """The rule by the existing one-frame entry: [(prev_k, curr_k)]."""
    p = [hs.preprocess_frame(f, fmt) for f in frames]
    return [(hs.preprocess_frame(p[k], "gray_blur") if reblurred(flags, k) else p[k], p[k + 1]) for k in range(len(frames) - 1)]


def host_sequence(hs, fmt, flags, views, W, H, dst_stride):
    """hsflow_preprocess_sequence_host on 2-D views of row bytes that share one stride, into padded planes of 0xA5."""
    n = len(views)
    prev = [np.full((H, dst_stride), 0xA5, np.uint8) for _ in range(n - 1)]
    curr = [np.full((H, dst_stride), 0xA5, np.uint8) for _ in range(n - 1)]
    src = (ctypes.c_void_p * n)(*[v.ctypes.data for v in views])
    pp = (ctypes.c_void_p * (n - 1))(*[a.ctypes.data for a in prev])
    pc = (ctypes.c_void_p * (n - 1))(*[a.ctypes.data for a in curr])
    st = hs._lib.load().hsflow_preprocess_sequence_host(hs._lib.FRAME_FORMATS[fmt], flags, src, n, views[0].strides[0], W, H, pp, pc, dst_stride)
    assert st == 0, st
    return prev, curr


def test_version_is_0_14(hs):
    assert hs._lib.load().hsflow_version() >= 14
    text = header()
    assert int(re.search(r"#define HSFLOW_VERSION_MINOR (\d+)", text).group(1)) >= 14
    assert int(re.search(r"#define HSFLOW_SEQ_REBLUR (\d+)", text).group(1)) == hs.SEQ_REBLUR == hs._lib.SEQ_REBLUR == 1
    assert int(re.search(r"#define HSFLOW_SEQ_REBLUR_FIRST (\d+)", text).group(1)) == hs.SEQ_REBLUR_FIRST == hs._lib.SEQ_REBLUR_FIRST == 2
    assert int(re.search(r"#define HSFLOW_PRE_SEQ_MAX (\d+)", text).group(1)) == hs.PRE_SEQ_MAX == hs._lib.PRE_SEQ_MAX >= 2
    assert "OpticalFlowOpenCV.cpp:76-93,118" in text


def test_new_prototypes_are_declared_bound_and_exported(hs):
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    declared = set(re.findall(r"\b(hsflow_[a-z0-9_]+)\s*\(", text))
    lib = ctypes.CDLL(hs._lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in hs._lib.PROTOTYPES and hasattr(lib, name), name
    assert callable(hs.preprocess_sequence) and hasattr(hs.HSFlow, "set_sequence_device")
    import inspect
    for method in (hs.HSFlow.set_sequence_device, hs.HSFlow.set_sequence_jpeg):
        names = inspect.signature(method).parameters
        assert "reblur" in names and "reblur_first" in names and "first_pair" in names
        assert names["reblur"].default is False and names["reblur_first"].default is False


def test_header_is_c99_and_links(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler is needed"
    src = tmp_path / "seq.c"
    src.write_text('#include "hsflow.h"\n#include <stdio.h>\n'
                   "int main(void)\n{\n"
                   "    const void *const frames[2] = {0, 0};\n"
                   "    const uint8_t *const files[2] = {0, 0};\n"
                   "    const size_t bytes[2] = {0, 0};\n"
                   "    uint8_t a[4] = {1, 2, 3, 4}, b[4] = {5, 6, 7, 8}, p[4], c[4];\n"
                   "    const uint8_t *const host[2] = {a, b};\n"
                   "    uint8_t *const prev[1] = {p}, *const curr[1] = {c};\n"
                   "    if (hsflow_set_sequence_device_ex(0, 0, HSFLOW_FRAMES_BGR8_BLUR, frames, 2, 0, HSFLOW_SEQ_REBLUR | HSFLOW_SEQ_REBLUR_FIRST) != HSFLOW_E_ARG) return 2;\n"
                   "    if (hsflow_set_sequence_jpeg_ex(0, 0, files, bytes, 2, 1, HSFLOW_SEQ_REBLUR) != HSFLOW_E_ARG) return 3;\n"
                   "    if (hsflow_preprocess_sequence_host(HSFLOW_FRAMES_GRAY8, 0, host, 2, 2, 2, 2, prev, curr, 2) != HSFLOW_OK) return 4;\n"
                   "    if (p[3] != 4 || c[0] != 5 || HSFLOW_PRE_SEQ_MAX < 2) return 5;\n"
                   "    return hsflow_version() >= 14 ? 0 : 7;\n}\n")
    exe = str(tmp_path / "seq")
    libdir = os.path.join(ROOT, "opticalflowhs_amd")
    r = subprocess.run([cc, "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe,
                        "-L", libdir, "-lhsflow", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])


def test_argument_errors_without_gpu(hs):
    L, E_ARG, E_SIZE = hs._lib.load(), hs._lib.E_ARG, hs._lib.E_SIZE
    buf = (ctypes.c_uint8 * 64)()
    two = (ctypes.c_void_p * 2)(ctypes.addressof(buf), ctypes.addressof(buf))
    sizes = (ctypes.c_size_t * 2)(64, 64)
    # the device entries: a null context comes back as an argument error, whatever else is passed
    assert L.hsflow_set_sequence_device_ex(None, 0, 3, two, 2, 64, 1) == E_ARG
    assert b"context" in L.hsflow_last_error(None)
    assert L.hsflow_set_sequence_device_ex(None, 0, 7, None, 1, 0, 2) == E_ARG
    assert L.hsflow_set_sequence_jpeg_ex(None, 0, two, sizes, 2, 1, 3) == E_ARG
    assert L.hsflow_set_sequence_jpeg_ex(None, -1, None, None, 0, 1, 5) == E_ARG
    # the host entry
    a, b = (ctypes.c_uint8 * 64)(), (ctypes.c_uint8 * 64)()
    holed = (ctypes.c_void_p * 2)(ctypes.addressof(buf), None)
    prev, curr, none = (ctypes.c_void_p * 1)(ctypes.addressof(a)), (ctypes.c_void_p * 1)(ctypes.addressof(b)), (ctypes.c_void_p * 1)(None)
    f = L.hsflow_preprocess_sequence_host
    assert f(3, 1, two, 2, 12, 4, 4, prev, curr, 4) == 0
    assert f(3, 1, None, 2, 12, 4, 4, prev, curr, 4) == E_ARG and f(3, 1, holed, 2, 12, 4, 4, prev, curr, 4) == E_ARG
    assert f(3, 1, two, 2, 12, 4, 4, None, curr, 4) == E_ARG and f(3, 1, two, 2, 12, 4, 4, prev, none, 4) == E_ARG
    assert f(4, 1, two, 2, 12, 4, 4, prev, curr, 4) == E_ARG and f(-1, 1, two, 2, 12, 4, 4, prev, curr, 4) == E_ARG
    for flags in (2, 4, -1, 5):
        assert f(3, flags, two, 2, 12, 4, 4, prev, curr, 4) == E_ARG, flags
    assert f(3, 0, two, 1, 12, 4, 4, prev, curr, 4) == E_ARG
    assert f(3, 0, two, 2, 11, 4, 4, prev, curr, 4) == E_SIZE and f(1, 0, two, 2, 3, 4, 4, prev, curr, 4) == E_SIZE
    assert f(3, 0, two, 2, 12, 4, 4, prev, curr, 3) == E_SIZE
    assert f(3, 0, two, 2, 12, 0, 4, prev, curr, 4) == E_SIZE and f(3, 0, two, 2, 12, 4, -1, prev, curr, 4) == E_SIZE
    with pytest.raises(ValueError):
        hs.preprocess_sequence([np.zeros((4, 4), np.uint8)] * 2, "bgr")
    with pytest.raises(hs.HsflowError) as e:
        hs.preprocess_sequence([np.zeros((4, 4), np.uint8)] * 2, "gray", reblur=False, reblur_first=True)
    assert e.value.status == E_ARG
    with pytest.raises(hs.HsflowError) as e:
        hs.preprocess_sequence([np.zeros((4, 4), np.uint8)], "gray")
    assert e.value.status == E_ARG


@pytest.mark.parametrize("fmt", FORMATS)
def test_host_rule_equals_compositions_of_the_frame_rule(hs, fmt):
    """Full-range noise, so that the rounding of p matters to B(p): every shape, flag set and frame count, dense through the
    Python mirror and, through the C entry, from bases at byte offsets 1 .. 3 with a padded stride into padded planes."""
    ch = 3 if fmt.startswith("bgr") else 1
    rng = np.random.default_rng(FORMATS.index(fmt))
    case = 0
    for W, H in SHAPES:
        for flags in FLAGS:
            for n in COUNTS:
                frames = [rng.integers(0, 256, (H, W, 3) if ch == 3 else (H, W), dtype=np.uint8) for _ in range(n)]
                want = composed(hs, frames, fmt, flags)
                got = hs.preprocess_sequence(frames, fmt, reblur=bool(flags & 1), reblur_first=bool(flags & 2))
                assert len(got) == n - 1
                for k in range(n - 1):
                    assert np.array_equal(got[k][0], want[k][0]) and np.array_equal(got[k][1], want[k][1]), (W, H, flags, n, k)
                off, pad = 1 + case % 3, 1 + case % 5
                case += 1
                stride = W * ch + pad
                views = []
                for f in frames:
                    raw = np.full(off + H * stride, 0x5A, np.uint8)         # padding must not leak into the result
                    view = raw[off:off + H * stride].reshape(H, stride)
                    view[:, :W * ch] = f.reshape(H, W * ch)
                    views.append(view)
                prev, curr = host_sequence(hs, fmt, flags, views, W, H, W + 3)
                for k in range(n - 1):
                    assert np.array_equal(prev[k][:, :W], want[k][0]) and np.array_equal(curr[k][:, :W], want[k][1]), (W, H, flags, n, k, off, pad)
                    assert np.all(prev[k][:, W:] == 0xA5) and np.all(curr[k][:, W:] == 0xA5), (W, H)


def box3(plane):
    """3x3 box blur of a plane with ITS OWN border repeated, rounded to nearest: numpy, independent of the library."""
    e = np.pad(plane.astype(np.int64), 1, mode="edge")
    H, W = plane.shape
    s = sum(e[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3))
    return ((2 * s + 9) // 18).astype(np.uint8)


@pytest.mark.parametrize("fmt", ["gray_blur", "bgr_blur"])
def test_the_double_blur_repeats_the_planes_own_border(hs, fmt):
    """Rows (then columns) alternating 0, 255, 0, 255 ...: B(p) row 0 needs p rows 0, 0, 1.  An implementation that clamps
    SOURCE row indices two rows out evaluates a p row "-1" from source rows 0, 0, 0 -- all 0 where p row 0 is 85 -- and
    gets the outermost rows and columns wrong."""
    for W, H in [(9, 12), (12, 9), (4, 3), (3, 4), (2, 2), (257, 10)]:
        for axis in (0, 1):
            ramp = (np.arange(H if axis == 0 else W) % 2 * 255).astype(np.uint8)
            g = np.repeat(ramp[:, None], W, 1) if axis == 0 else np.repeat(ramp[None, :], H, 0)
            f = np.repeat(g[:, :, None], 3, 2) if fmt == "bgr_blur" else g   # B = G = R: the gray formula gives the value back
            f = np.ascontiguousarray(f)
            assert np.array_equal(hs.preprocess_frame(f, fmt), box3(g))
            want = box3(box3(g))
            wrong = box3(np.pad(g, 2, mode="edge"))          # clamped source two out, blurred twice without re-clamping p
            wrong = box3(wrong)[2:-2, 2:-2]
            got = hs.preprocess_sequence([f, f, f], fmt, reblur=True)[1][0]
            for name, sl in (("row 0", np.s_[0, :]), ("row H-1", np.s_[H - 1, :]), ("column 0", np.s_[:, 0]), ("column W-1", np.s_[:, W - 1])):
                assert np.array_equal(got[sl], want[sl]), (W, H, axis, name)
            assert np.array_equal(got, want), (W, H, axis)
            if (H if axis == 0 else W) >= 3:
                assert not np.array_equal(wrong, want), "the case must be able to tell the two apart"
            first = hs.preprocess_sequence([f, f, f], fmt, reblur=True, reblur_first=True)
            assert np.array_equal(first[0][0], want) and np.array_equal(first[1][0], want)
            assert np.array_equal(hs.preprocess_sequence([f, f, f], fmt, reblur=True)[0][0], box3(g))


def test_rule_header_alone_under_sanitizers(tmp_path):
    """csrc/hs_pre_rule.h and nothing else, compiled for the host with AddressSanitizer and UBSan into a program of its own
    (tests/pre_sequence_asan_main.cpp): sources allocated exactly to size, guard bytes around every output plane.  The
    sanitizer runtimes are linked into the program statically; nothing of it is loaded into Python."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the stand-alone rule check"
    S = int(re.search(r"#define HSFLOW_PRE_STRIP_ROWS (\d+)", header()).group(1))
    exe = str(tmp_path / "pre_sequence_asan")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                        "-I", os.path.join(ROOT, "opticalflowhs_amd", "csrc"), os.path.join(ROOT, "tests", "pre_sequence_asan_main.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, str(S)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    assert "pre sequence ok" in r.stdout and ("strip rows %d" % S) in r.stdout
