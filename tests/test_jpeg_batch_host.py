"""The batched JPEG encode without a device (include/hsflow.h, ABI 0.13): the version, the header's declarations, the
symbols and their null checks, the Python mirrors, and the batch layout (opticalflowhs_amd/csrc/hs_jpeg_batch_plan.h)
as a program of its own under AddressSanitizer and UBSan."""
import ctypes
import os
import re
import shutil
import subprocess

from conftest import ROOT

E_ARG = 1
ENTRIES = ("hsflow_jpeg_encode_batch_device", "hsflow_render_flow_batch_device", "hsflow_render_flow_jpeg_batch_device",
           "hsflow_render_flow_jpeg_batch")


def header_text():
    with open(os.path.join(ROOT, "include", "hsflow.h")) as f:
        return f.read()


def batch_max():
    m = re.search(r"^#define HSFLOW_JPEG_BATCH_MAX\s+(\d+)", header_text(), re.M)
    assert m, "include/hsflow.h does not define HSFLOW_JPEG_BATCH_MAX"
    return int(m.group(1))


def test_version_and_header(hs):
    L = hs._lib.load()
    assert L.hsflow_version() >= 13
    text = header_text()
    for name in ENTRIES:
        assert re.search(r"^int %s\(" % name, text, re.M), name
    assert batch_max() in (4, 8, 16, 32)
    assert hs._lib.JPEG_BATCH_MAX == batch_max() == hs.JPEG_BATCH_MAX
    # the reference lines the entries stand for
    assert "OpticalFlowOpenCV.cpp:32-47" in text and "HSOpticalFlowOpenCL.cpp:759-771" in text


def test_symbols_and_null_handles(hs):
    L = hs._lib.load()
    blob = (ctypes.c_uint8 * 64)(*([0xA5] * 64))
    lists = (ctypes.c_void_p * 2)(ctypes.addressof(blob), ctypes.addressof(blob) + 32)
    words = (ctypes.c_uint64 * 2)(77, 77)
    sizes = (ctypes.c_size_t * 2)(77, 77)
    rp = hs.make_render_params("cv")
    assert L.hsflow_jpeg_encode_batch_device(None, lists, 2, 24, 95, lists, 32, words) == E_ARG
    assert L.hsflow_render_flow_batch_device(None, 0, 2, ctypes.byref(rp), lists, 24) == E_ARG
    assert L.hsflow_render_flow_jpeg_batch_device(None, 0, 2, ctypes.byref(rp), 95, lists, 32, words) == E_ARG
    assert L.hsflow_render_flow_jpeg_batch(None, 0, 2, ctypes.byref(rp), 95, lists, 32, sizes) == E_ARG
    assert b"null context" in L.hsflow_last_error(None)
    assert list(words) == [77, 77] and list(sizes) == [77, 77] and bytes(blob) == b"\xa5" * 64


def test_python_mirrors(hs):
    for name in ("encode_jpeg_batch", "render_jpeg_batch", "render_batch_device"):
        assert callable(getattr(hs.HSFlow, name)), name


def test_batch_layout_alone_under_sanitizers(tmp_path):
    """csrc/hs_jpeg_batch_plan.h and nothing else, compiled for the host with AddressSanitizer and UBSan into a program of
    its own (tests/jpeg_batch_plan_main.cpp), the sanitizer runtimes linked statically: it runs as it is."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the stand-alone layout check"
    exe = str(tmp_path / "jpeg_batch_plan")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                        "-I", os.path.join(ROOT, "opticalflowhs_amd", "csrc"), os.path.join(ROOT, "tests", "jpeg_batch_plan_main.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, str(batch_max())], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    m = re.search(r"batch plan ok: (\d+) layouts, (\d+) sizes, maximum %d" % batch_max(), r.stdout)
    assert m and int(m.group(1)) >= 2 * 259 * 3 * batch_max() and int(m.group(2)) == 259, r.stdout[-500:]
