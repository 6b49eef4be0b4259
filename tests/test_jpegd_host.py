"""The JPEG decoding rule on the host (include/hsflow.h: hsflow_jpeg_read_header, hsflow_jpeg_decode_host;
csrc/hs_jpegd_rule.h) against PIL's pixels committed next to the fixtures of tests/golden/jpegd, against the CLI's reader
(csrc/host/jpeg_baseline.hpp through jpeg2ppm, itself held to libjpeg-turbo by tests/test_jpeg.py), and on the reference's
own input files against the committed gray planes.  The device decoder is compiled from the same header and checked
against this host form in tests/test_gpu_jpegd.py.  CPU-only."""
import ctypes
import hashlib
import io
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import jpegd_cases as jc
import refpics
from conftest import GOLDEN, ROOT
from jpegd_cases import BGR, E_ARG, E_DATA, E_SIZE, OK, RGB

NEW = ["hsflow_jpeg_read_header", "hsflow_jpeg_decode_host", "hsflow_jpeg_decode_device", "hsflow_jpeg_decode", "hsflow_set_frames_jpeg",
       "hsflow_push_frame_jpeg"]
CSRC = os.path.join(ROOT, "opticalflowhs_amd", "csrc")


def header_text():
    return open(os.path.join(ROOT, "include", "hsflow.h")).read()


@pytest.fixture(scope="module")
def jpeg2ppm(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the yardstick"
    exe = str(tmp_path_factory.mktemp("jpegd") / "jpeg2ppm")
    r = subprocess.run([gxx, "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(CSRC, "host", "jpeg2ppm.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def rule_main(tmp_path_factory):
    """tests/jpegd_rule_main.cpp with AddressSanitizer and UBSan linked in statically: a program of its own."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the stand-alone rule check"
    exe = str(tmp_path_factory.mktemp("jpegd_rule") / "jpegd_rule_san")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                        "-static-libubsan", "-I", CSRC, os.path.join(ROOT, "tests", "jpegd_rule_main.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def cli_reader(exe, blob, tmp):
    src, out = os.path.join(tmp, "i.jpg"), os.path.join(tmp, "o.ppm")
    with open(src, "wb") as f:
        f.write(blob)
    r = subprocess.run([exe, src, out], capture_output=True, text=True)
    if r.returncode != 0:
        return None
    with open(out, "rb") as f:
        magic = f.readline().strip()
        w, h = [int(t) for t in f.readline().split()]
        f.readline()
        a = np.frombuffer(f.read(), np.uint8)
    return a.reshape(h, w, 3) if magic == b"P6" else np.repeat(a.reshape(h, w)[:, :, None], 3, axis=2)


def test_abi(hs):
    L = hs._lib.load()
    assert L.hsflow_version() >= 11
    h = header_text()
    assert int(re.search(r"#define HSFLOW_VERSION_MINOR (\d+)", h).group(1)) >= 11
    assert re.search(r"#define HSFLOW_E_DATA 7\b", h) and hs._lib.E_DATA == 7
    assert int(re.search(r"#define HSFLOW_JPEGD_SUBSEQ_BITS (\d+)", h).group(1)) == hs._lib.JPEGD_SUBSEQ_BITS
    assert hs._lib.JPEGD_SUBSEQ_BITS % 32 == 0 and 32 <= hs._lib.JPEGD_SUBSEQ_BITS <= 4096
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, h), name
        assert name in hs._lib.PROTOTYPES and hasattr(L, name), name
    assert L.hsflow_status_string(7) not in (b"unknown status", None)
    assert ctypes.sizeof(hs._lib.HsflowJpegInfo) == 56


def test_header_compiles_as_c99(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler is needed"
    src = tmp_path / "abi.c"
    src.write_text('#include "hsflow.h"\nint main(void) { hsflow_jpeg_info i; i.struct_size = sizeof i; return HSFLOW_E_DATA == 7 && i.struct_size == 56 ? 0 : 1; }\n')
    r = subprocess.run([cc, "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "abi")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert subprocess.run([str(tmp_path / "abi")]).returncode == 0


def test_rule_header_compiles_alone(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed"
    src = tmp_path / "alone.cpp"
    src.write_text('#include "hs_jpegd_rule.h"\nint main() { return hsjpegd::byte_class(0xFF, 0xD3, 0) == 2 && hsjpegd::extend(0, 3) == -7 ? 0 : 1; }\n')
    r = subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, str(src), "-o", str(tmp_path / "alone")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert subprocess.run([str(tmp_path / "alone")]).returncode == 0


def test_fixtures_are_the_committed_ones():
    names = jc.names()
    assert len(names) == 16
    lines = open(os.path.join(jc.DIR, "SHA256SUMS")).read().split()
    sums = dict(zip(lines[1::2], lines[0::2]))
    assert set(sums) == {n + ".jpg" for n in names} | {"pixels.npz"}
    for name, digest in sums.items():
        assert hashlib.sha256(open(os.path.join(jc.DIR, name), "rb").read()).hexdigest() == digest, name


def test_headers(hs):
    seen = set()
    for name in jc.names():
        st, info = jc.header(hs, jc.data(name))
        assert st == OK, name
        want = jc.pil_pixels(name)
        assert (info.height, info.width) == want.shape[:2], name
        assert info.components == (1 if name.startswith("g") else 3)
        samp = {"444": (1, 1), "422": (2, 1), "420": (2, 2)}.get(name.split("_")[1], (1, 1))
        assert (info.h_samp, info.v_samp) == samp, name
        assert (info.restart_interval > 0) == ("rst" in name), name
        assert info.subseq_bits == (0 if info.restart_interval else hs._lib.JPEGD_SUBSEQ_BITS)
        mx, my = -(-info.width // (8 * samp[0])), -(-info.height // (8 * samp[1]))
        assert info.blocks == mx * my * (1 if info.components == 1 else samp[0] * samp[1] + 2)
        blob = jc.data(name)
        assert blob[info.scan_offset + info.scan_bytes:] == b"\xff\xd9" and blob[info.scan_offset - 14 if info.components == 3 else info.scan_offset - 10] == 0xFF
        seen.add((info.components, samp, info.restart_interval > 0))
    assert len(seen) >= 6
    assert hs.jpeg_read_header(jc.data("c17x9_420_q75_noise"))["width"] == 17


def test_host_twin_is_pil(hs):
    for name in jc.names():
        want = jc.pil_pixels(name)
        for order in (RGB, BGR):
            st, info, rows = jc.decode_host_raw(hs, jc.data(name), order, pad=(0, 5, 8)[len(name) % 3])
            assert st == OK, name
            H, W = want.shape[:2]
            got = rows[:, :3 * W].reshape(H, W, 3)
            assert np.array_equal(got if order == RGB else got[:, :, ::-1], want), (name, order)
            assert (rows[:, 3 * W:] == 0xA5).all(), name
        assert np.array_equal(hs.jpeg_decode_host(jc.data(name)), want)
        assert np.array_equal(hs.jpeg_decode_host(jc.data(name), "bgr"), want[:, :, ::-1])


def test_host_twin_is_the_cli_reader(hs, jpeg2ppm, tmp_path):
    for blob in [jc.data(n) for n in jc.names()] + [jc.golden(n) for n in jc.REFERENCE_INPUTS]:
        want = cli_reader(jpeg2ppm, blob, str(tmp_path))
        assert want is not None
        assert np.array_equal(hs.jpeg_decode_host(blob), want)


def test_reference_inputs_give_the_committed_gray_planes(hs):
    for name in ("city", "bunny"):
        for k in (1, 2):
            bgr = hs.jpeg_decode_host(jc.golden("ref_%s_%d.jpg" % (name, k)), "bgr")
            assert np.array_equal(hs.preprocess_frame(bgr, "bgr"), refpics.read_pgm(os.path.join(GOLDEN, "%s_%d_gray.pgm" % (name, k)))), (name, k)


def test_synthetic_files_decode_like_pil(hs):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(5)
    for case in range(200):
        W = int(rng.integers(1, 90)) if case % 3 else int(rng.integers(1, 20))
        H = int(rng.integers(1, 70)) if case % 4 else int(rng.integers(1, 18))
        gray = case % 7 == 0
        kind = case % 3
        if kind == 0:
            arr = rng.integers(0, 256, size=(H, W) if gray else (H, W, 3), dtype=np.uint8)
        elif kind == 1:
            yy, xx = np.mgrid[0:H, 0:W]
            base = (xx * 3 + yy * 2) % 256
            arr = base.astype(np.uint8) if gray else np.stack([base, (base * 2) % 256, 255 - base], axis=2).astype(np.uint8)
        else:
            arr = np.full((H, W) if gray else (H, W, 3), 40, np.uint8)
            arr[H // 3:H // 3 + max(1, H // 4), W // 3:W // 3 + max(1, W // 4)] = 230
        kw = dict(quality=int(rng.choice([20, 50, 75, 90, 95, 100])), optimize=bool(case % 2))
        if not gray:
            kw["subsampling"] = int(rng.choice([0, 1, 2]))
        if case % 5 == 0:
            kw["restart_marker_blocks"] = int(rng.integers(1, 6))
        buf = io.BytesIO()
        try:
            Image.fromarray(arr).save(buf, format="JPEG", **kw)
        except (TypeError, OSError):
            kw.pop("restart_marker_blocks", None)
            buf = io.BytesIO()
            Image.fromarray(arr).save(buf, format="JPEG", **kw)
        ref = np.asarray(Image.open(io.BytesIO(buf.getvalue())))
        ref = ref if ref.ndim == 3 else np.repeat(ref[:, :, None], 3, axis=2)
        assert np.array_equal(hs.jpeg_decode_host(buf.getvalue()), ref), (case, W, H, gray, kw)


def test_encoder_round_trip(hs):
    """Files written by hsflow_jpeg_encode_host through the twin: PIL's pixels where PIL is there, and in any case the
    CLI reader's agreement is covered above -- here the twin must at least reproduce a flat picture exactly."""
    flat = np.full((20, 37, 3), 128, np.uint8)
    assert np.array_equal(hs.jpeg_decode_host(hs.encode_jpeg(flat, 95)), flat)
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(11)
    for W, H, q in ((1, 1, 95), (16, 16, 95), (37, 20, 30), (80, 60, 75), (33, 47, 100)):
        blob = hs.encode_jpeg(rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8), q)
        assert np.array_equal(hs.jpeg_decode_host(blob), np.asarray(Image.open(io.BytesIO(blob)))), (W, H, q)


def _patch_sof(blob, fn):
    b = bytearray(blob)
    i = b.index(b"\xff\xc0")
    ln = (b[i + 2] << 8) | b[i + 3]
    seg = fn(bytearray(b[i + 4:i + 2 + ln]))
    return bytes(b[:i + 4]) + bytes(seg) + bytes(b[i + 2 + ln:])


def _set(seg, pos, val):
    seg[pos] = val
    return seg


def test_refusals(hs):
    good, gray = jc.data("c33x31_420_q95_noise_rst3_opt"), jc.data("g33x31_q95_noise_rst3")
    plain = jc.data("c64x48_420_q95_noise")
    i = good.index(b"\xff\xc0")
    sof = good[i:i + 4 + ((good[i + 2] << 8) | good[i + 3]) - 2]
    j = good.index(b"\xff\xda")
    cases = {
        "progressive": good[:i] + b"\xff\xc2" + good[i + 2:],
        "arithmetic": good[:i] + b"\xff\xc9" + good[i + 2:],
        "twelve_bit": _patch_sof(good, lambda s: _set(s, 0, 12)),
        "not_jpeg": b"P6\n1 1\n255\n\x00\x00\x00",
        "empty": b"",
        "cut3": good[:3], "cut20": good[:20], "cut_third_of_header": good[:j // 3],
        "zero_h": _patch_sof(good, lambda s: _set(s, 7, 0x02)), "zero_v": _patch_sof(good, lambda s: _set(s, 7, 0x20)),
        "zero_chroma": _patch_sof(good, lambda s: _set(s, 10, 0x00)), "gray_zero": _patch_sof(gray, lambda s: _set(s, 7, 0x00)),
        "h3": _patch_sof(good, lambda s: _set(s, 7, 0x32)), "h4v4": _patch_sof(good, lambda s: _set(s, 7, 0x44)), "h1v2": _patch_sof(good, lambda s: _set(s, 7, 0x12)),
        "chroma_2x1": _patch_sof(good, lambda s: _set(s, 10, 0x21)),
        "double_sof": good[:i] + sof + good[i:],
        "two_components": _patch_sof(good, lambda s: _set(s, 5, 2)),
        "sos_len2": good[:j] + b"\xff\xda\x00\x02" + good[j + 4:], "sos_len2_eof": good[:j] + b"\xff\xda\x00\x02", "sos_len3_eof": good[:j] + b"\xff\xda\x00\x03\x03",
        "zero_dims": _patch_sof(good, lambda s: s[:1] + bytes(4) + s[5:]),
        "missing_dht": good[:good.index(b"\xff\xc4")] + good[i:] if good.index(b"\xff\xc4") < i else good[:good.index(b"\xff\xc4")] + good[j:],
        "missing_dqt": good[:good.index(b"\xff\xdb")] + good[min(i, good.index(b"\xff\xc4")):],
        "no_scan": good[:j] + b"\xff\xd9",
    }
    for name, blob in cases.items():
        st, _ = jc.header(hs, blob) if blob else (hs._lib.load().hsflow_jpeg_read_header(ctypes.c_void_p(np.zeros(1, np.uint8).ctypes.data), 0, ctypes.byref(jc.info_struct(hs))), None)
        assert st == E_DATA, name
        st, _, rows = jc.decode_host_raw(hs, blob)
        assert st == E_DATA and (rows == 0xA5).all(), name
        assert b"JPEG file" in hs._lib.load().hsflow_last_error(None)
    # the entropy-coded data: cut, and a run past 63
    for blob in (plain, good):
        off, n = jc.scan_range(hs, blob)
        for keep in (n // 4, n // 2, n - 3):
            st, info, rows = jc.decode_host_raw(hs, jc.cut_scan(hs, blob, keep))
            assert st == E_DATA and (rows == 0xA5).all() and info.width in (33, 64), keep
            assert b"truncated" in hs._lib.load().hsflow_last_error(None), keep
        assert jc.decode_host_raw(hs, jc.cut_scan(hs, blob, n))[0] == OK
    st, _, rows = jc.decode_host_raw(hs, jc.run_past_63(hs, jc.data("g8x8_q75_smooth")))
    assert st == E_DATA and b"corrupt" in hs._lib.load().hsflow_last_error(None) and (rows == 0xA5).all()
    with pytest.raises(hs.HsflowError) as e:
        hs.jpeg_decode_host(cases["progressive"])
    assert e.value.status == E_DATA
    # arguments
    L = hs._lib.load()
    buf = np.frombuffer(plain, np.uint8)
    pix = np.zeros((48, 64 * 3), np.uint8)
    f, p, o = L.hsflow_jpeg_decode_host, ctypes.c_void_p(buf.ctypes.data), ctypes.c_void_p(pix.ctypes.data)
    assert f(p, buf.size, RGB, o, 192, None) == OK
    assert f(None, buf.size, RGB, o, 192, None) == E_ARG and f(p, buf.size, RGB, None, 192, None) == E_ARG
    assert f(p, buf.size, 2, o, 192, None) == E_ARG and f(p, buf.size, -1, o, 192, None) == E_ARG
    assert f(p, buf.size, RGB, o, 191, None) == E_SIZE and b"stride" in L.hsflow_last_error(None)
    bad = jc.info_struct(hs)
    bad.struct_size = 8
    assert f(p, buf.size, RGB, o, 192, ctypes.byref(bad)) == E_ARG and L.hsflow_jpeg_read_header(p, buf.size, ctypes.byref(bad)) == E_ARG
    assert L.hsflow_jpeg_read_header(None, 4, ctypes.byref(jc.info_struct(hs))) == E_ARG and L.hsflow_jpeg_read_header(p, buf.size, None) == E_ARG
    st = ctypes.c_uint32()
    assert L.hsflow_jpeg_decode_device(None, p, buf.size, RGB, o, 192, ctypes.byref(st)) == E_ARG
    assert L.hsflow_jpeg_decode(None, p, buf.size, RGB, o, 192) == E_ARG
    assert L.hsflow_set_frames_jpeg(None, 0, p, buf.size, p, buf.size, 1) == E_ARG and L.hsflow_push_frame_jpeg(None, 0, p, buf.size, 1, 0) == E_ARG


def test_flipped_scan_bytes_never_crash(hs):
    rng = np.random.default_rng(3)
    for name in ("c64x48_420_q95_noise", "c48x40_422_q75_noise_rst7", "g250x130_q30_noise_opt"):
        blob = jc.data(name)
        off, n = jc.scan_range(hs, blob)
        want = jc.pil_pixels(name)
        outcomes = set()
        for _ in range(150):
            b = bytearray(blob)
            b[off + int(rng.integers(0, n))] ^= 1 << int(rng.integers(0, 8))
            st, _, rows = jc.decode_host_raw(hs, bytes(b), shape=want.shape[:2])
            assert st in (OK, E_DATA), name
            assert st == OK or (rows == 0xA5).all()
            outcomes.add(st)
        assert outcomes == {OK, E_DATA}, name


def test_rule_header_alone_under_sanitizers(rule_main):
    """Parse and decode over every fixture, and over all single-byte truncations and 2 000 seeded bit flips of three of
    them, on buffers allocated exactly: no report.  A child process; nothing of it is loaded into Python."""
    paths = [os.path.join(jc.DIR, n + ".jpg") for n in ["g8x8_q75_smooth", "c17x9_420_q75_noise", "c33x31_420_q95_noise_rst3_opt"] + jc.names()]
    r = subprocess.run([rule_main, "all"] + paths, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    assert "jpegd rule ok: 19 files" in r.stdout


@pytest.mark.parametrize("S", [32, 64, 1024])
def test_speculative_decode_is_the_sequential_one(rule_main, S):
    """The device decoder's procedure from the rule header, on the host: for every fixture without restart intervals (and
    the reference's inputs) the rounds reach the sequential decode's exit states and the write pass its coefficients."""
    paths = [os.path.join(jc.DIR, n + ".jpg") for n in jc.names()] + [os.path.join(GOLDEN, n) for n in jc.REFERENCE_INPUTS]
    r = subprocess.run([rule_main, "spec", str(S)] + paths, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    assert re.search(r"jpegd spec ok: S=%d, 16 files" % S, r.stdout), r.stdout
