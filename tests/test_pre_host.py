"""CPU checks of the device-resident pre-processing (ABI 0.9): the new entry points exist and refuse bad arguments without
a GPU, and the row rule of csrc/hs_pre_rule.h -- the one header the fused kernel and `hsflow_preprocess_frame_host` are
compiled from -- equals the CPU oracle's BGR->gray and 3x3 box blur bit for bit, clamps included."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NEW = ["hsflow_set_frames_device_ex", "hsflow_push_frame_ex", "hsflow_push_frame_device_ex", "hsflow_pipeline_submit_device_ex",
       "hsflow_preprocess_frame_host"]
WIDTHS = [1, 2, 3, 4, 5, 7, 255, 256, 257, 260]


def header():
    return open(os.path.join(ROOT, "include", "hsflow.h")).read()


def strip_rows():
    return int(re.search(r"#define HSFLOW_PRE_STRIP_ROWS (\d+)", header()).group(1))


def heights():
    S = strip_rows()
    return sorted({1, 2, 3, S - 1, S, S + 1, 2 * S + 1} - {0})


def oracle_pre(oracle, img, frames):
    g = oracle.bgr2gray(np.ascontiguousarray(img)) if frames.startswith("bgr") else np.ascontiguousarray(img)
    return oracle.box_blur3(g) if frames.endswith("blur") else g


def host_rule(hs, fmt, src, width, height, dst=None, dst_stride=None):
    """hsflow_preprocess_frame_host on a (possibly strided, possibly misaligned) 2-D view of row bytes."""
    out = np.full((height, dst_stride or width), 0xA5, np.uint8) if dst is None else dst
    st = hs._lib.load().hsflow_preprocess_frame_host(fmt, ctypes.c_void_p(src.ctypes.data), src.strides[0], width, height,
                                                     ctypes.c_void_p(out.ctypes.data), out.strides[0])
    assert st == 0, st
    return out


def test_version_is_0_9(hs):
    assert hs._lib.load().hsflow_version() >= 9
    assert int(re.search(r"#define HSFLOW_VERSION_MINOR (\d+)", header()).group(1)) >= 9
    assert hs.PRE_STRIP_ROWS == hs._lib.PRE_STRIP_ROWS == strip_rows() >= 2


def test_new_prototypes_are_declared_bound_and_exported(hs):
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    declared = set(re.findall(r"\b(hsflow_[a-z0-9_]+)\s*\(", text))
    lib = ctypes.CDLL(hs._lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in hs._lib.PROTOTYPES, name
    for name in declared:
        assert hasattr(lib, name), name
    assert callable(hs.preprocess_frame) and hasattr(hs.HSFlow, "set_frames_device") and hasattr(hs.HSFlow, "push_frame_ex")


def test_argument_errors_without_gpu(hs):
    L, E_ARG, E_SIZE = hs._lib.load(), hs._lib.E_ARG, hs._lib.E_SIZE
    buf = (ctypes.c_uint8 * 64)()
    out = (ctypes.c_uint8 * 64)()
    p = hs.make_params()
    assert L.hsflow_set_frames_device_ex(None, 0, 3, buf, 64, buf, 64) == E_ARG
    assert L.hsflow_set_frames_device_ex(None, 0, 0, buf, 64, buf, 64) == E_ARG
    assert L.hsflow_push_frame_ex(None, 0, 1, buf, 64, 1) == E_ARG
    assert L.hsflow_push_frame_device_ex(None, 0, 1, buf, 64, 1) == E_ARG
    assert L.hsflow_pipeline_submit_device_ex(None, 3, buf, 64, buf, 64, ctypes.byref(p), None) == E_ARG
    assert L.hsflow_pipeline_submit_device_ex(None, 0, buf, 64, buf, 64, ctypes.byref(p), None) == E_ARG
    f = L.hsflow_preprocess_frame_host
    assert f(1, None, 8, 8, 8, out, 8) == E_ARG and f(1, buf, 8, 8, 8, None, 8) == E_ARG
    assert f(4, buf, 8, 8, 8, out, 8) == E_ARG and f(-1, buf, 8, 8, 8, out, 8) == E_ARG
    assert b"format" in L.hsflow_last_error(None)
    assert f(1, buf, 8, 0, 8, out, 8) == E_SIZE and f(1, buf, 8, 8, -1, out, 8) == E_SIZE
    assert f(1, buf, 7, 8, 8, out, 8) == E_SIZE      # gray stride < width
    assert f(3, buf, 11, 4, 4, out, 4) == E_SIZE     # colour stride < 3 * width
    assert f(2, buf, 12, 4, 4, out, 3) == E_SIZE     # destination stride < width
    assert f(3, buf, 12, 4, 4, out, 4) == 0
    with pytest.raises(ValueError):
        hs.preprocess_frame(np.zeros((4, 4), np.uint8), "bgr")
    with pytest.raises(KeyError):
        hs.preprocess_frame(np.zeros((4, 4), np.uint8), "rgb")


@pytest.mark.parametrize("frames", ["gray_blur", "bgr", "bgr_blur"])
def test_host_rule_equals_the_oracle(hs, oracle, frames):
    """Random frames of every width and height of the list, dense through the Python mirror and, through the C entry,
    with a padded source stride from a base at byte offsets 1, 2 and 3 into a padded destination."""
    fmt = hs._lib.FRAME_FORMATS[frames]
    ch = 3 if fmt >= hs._lib.FRAMES_BGR8 else 1
    rng = np.random.default_rng(fmt)
    case = 0
    for W in WIDTHS:
        for H in heights():
            img = rng.integers(0, 256, (H, W, 3) if ch == 3 else (H, W), dtype=np.uint8)
            want = oracle_pre(oracle, img, frames)
            assert np.array_equal(hs.preprocess_frame(img, frames), want), (W, H)
            off, pad = 1 + case % 3, 1 + case % 5
            case += 1
            stride = W * ch + pad
            raw = np.zeros(off + H * stride, np.uint8)
            view = raw[off:off + H * stride].reshape(H, stride)
            view[:, :W * ch] = img.reshape(H, W * ch)
            view[:, W * ch:] = 0x5A                         # padding must not leak into the result
            out = host_rule(hs, fmt, view, W, H, dst_stride=W + 3)
            assert np.array_equal(out[:, :W], want), (W, H, off, pad)
            assert np.all(out[:, W:] == 0xA5), (W, H)


@pytest.mark.parametrize("value", [0, 255])
def test_host_rule_on_flat_frames(hs, oracle, value):
    """All 0 and all 255: the two ends of the rounding division (sum 0 and sum 9 * 255) and of the gray formula."""
    S = strip_rows()
    for W, H in [(1, 1), (5, 3), (257, S + 1), (260, 2 * S + 1)]:
        for frames in ("gray_blur", "bgr", "bgr_blur"):
            img = np.full((H, W, 3) if frames.startswith("bgr") else (H, W), value, np.uint8)
            got = hs.preprocess_frame(img, frames)
            assert np.array_equal(got, oracle_pre(oracle, img, frames)) and np.all(got == value), (W, H, frames)


def test_blurring_twice(hs, oracle):
    rng = np.random.default_rng(9)
    S = strip_rows()
    for W, H in [(7, 3), (255, S), (257, 2 * S + 1)]:
        g = rng.integers(0, 256, (H, W), dtype=np.uint8)
        once = hs.preprocess_frame(g, "gray_blur")
        assert np.array_equal(hs.preprocess_frame(once, "gray_blur"), oracle.box_blur3(oracle.box_blur3(g)))
        assert np.array_equal(hs.preprocess_frame(g, "gray"), g)


def test_rule_header_alone_under_sanitizers(tmp_path):
    """csrc/hs_pre_rule.h and nothing else, compiled for the host with AddressSanitizer and UBSan into a program of its own
    that runs the shapes above on buffers allocated exactly to size (tests/pre_rule_asan_main.cpp).  The sanitizer runtimes
    are linked into the program statically: it runs as it is, whatever else the environment loads into a process."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the stand-alone rule check"
    exe = str(tmp_path / "pre_rule_asan")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                        "-I", os.path.join(ROOT, "opticalflowhs_amd", "csrc"), os.path.join(ROOT, "tests", "pre_rule_asan_main.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, str(strip_rows())], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    assert "pre rule ok" in r.stdout and ("strip rows %d" % strip_rows()) in r.stdout
