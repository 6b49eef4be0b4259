"""The batched JPEG decode without a device (include/hsflow.h, ABI 0.12): the version, the header's declarations, the
symbols and their null checks, the Python mirrors, and the batch layout (opticalflowhs_amd/csrc/hs_jpegd_batch_plan.h)
as a program of its own under AddressSanitizer and UBSan."""
import ctypes
import os
import re
import shutil
import subprocess

from conftest import ROOT

E_ARG = 1
ENTRIES = ("hsflow_jpeg_decode_batch_device", "hsflow_set_sequence_jpeg", "hsflow_pipeline_submit_jpeg")


def header_text():
    with open(os.path.join(ROOT, "include", "hsflow.h")) as f:
        return f.read()


def batch_max():
    m = re.search(r"^#define HSFLOW_JPEGD_BATCH_MAX\s+(\d+)", header_text(), re.M)
    assert m, "include/hsflow.h does not define HSFLOW_JPEGD_BATCH_MAX"
    return int(m.group(1))


def test_version_and_header(hs):
    L = hs._lib.load()
    assert L.hsflow_version() >= 12
    text = header_text()
    for name in ENTRIES:
        assert re.search(r"^int %s\(" % name, text, re.M), name
    assert batch_max() in (4, 8, 16, 32)
    assert hs._lib.JPEGD_BATCH_MAX == batch_max() == hs.JPEGD_BATCH_MAX
    # the reference lines each entry stands for
    assert "OpticalFlowOpenCV.cpp:15,18" in text and ":76,83" in text


def test_symbols_and_null_handles(hs):
    L = hs._lib.load()
    blob = (ctypes.c_uint8 * 4)(0xFF, 0xD8, 0xFF, 0xD9)
    files = (ctypes.c_void_p * 2)(ctypes.addressof(blob), ctypes.addressof(blob))
    sizes = (ctypes.c_size_t * 2)(4, 4)
    pix = (ctypes.c_void_p * 2)(0, 0)
    assert L.hsflow_jpeg_decode_batch_device(None, files, sizes, 2, 0, pix, 0, None) == E_ARG
    assert L.hsflow_set_sequence_jpeg(None, 0, files, sizes, 2, 1) == E_ARG
    assert L.hsflow_set_frames_jpeg_async(None, 0, files[0], 4, files[1], 4, 1) == E_ARG
    assert L.hsflow_jpeg_async_status(None) == E_ARG
    p = hs.make_params(lam=1.0, max_iter=1, term_type=hs.TERM_ITER)
    t = ctypes.c_uint64(77)
    assert L.hsflow_pipeline_submit_jpeg(None, files[0], 4, files[1], 4, 1, ctypes.byref(p), ctypes.byref(t)) == E_ARG
    assert t.value == 77


def test_python_mirrors(hs):
    for name in ("jpeg_decode_batch", "set_sequence_jpeg"):
        assert callable(getattr(hs.HSFlow, name)), name
    assert callable(hs.PairPipeline.submit_jpeg)


def test_batch_layout_alone_under_sanitizers(tmp_path):
    """csrc/hs_jpegd_batch_plan.h and nothing else, compiled for the host with AddressSanitizer and UBSan into a program of
    its own (tests/jpegd_batch_plan_main.cpp), the sanitizer runtimes linked statically: it runs as it is."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the stand-alone layout check"
    exe = str(tmp_path / "jpegd_batch_plan")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                        "-I", os.path.join(ROOT, "opticalflowhs_amd", "csrc"), os.path.join(ROOT, "tests", "jpegd_batch_plan_main.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, str(batch_max())], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    m = re.search(r"batch plan ok: (\d+) batches, maximum %d" % batch_max(), r.stdout)
    assert m and int(m.group(1)) >= 300, r.stdout[-500:]
