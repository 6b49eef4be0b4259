"""What tests/test_jpegd_host.py and tests/test_gpu_jpegd.py share: the committed fixtures of tests/golden/jpegd with
PIL's pixels, the raw ctypes calls, and the ways a good file is broken."""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
DIR = os.path.join(GOLDEN, "jpegd")
OK, E_ARG, E_SIZE, E_DATA = 0, 1, 2, 7
BGR, RGB = 0, 1
REFERENCE_INPUTS = ["ref_city_1.jpg", "ref_city_2.jpg", "ref_bunny_1.jpg", "ref_bunny_2.jpg"]


def names():
    return sorted(n[:-4] for n in os.listdir(DIR) if n.endswith(".jpg"))


def data(name):
    with open(os.path.join(DIR, name + ".jpg"), "rb") as f:
        return f.read()


def golden(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


_pixels = None


def pil_pixels(name):
    """(H, W, 3) RGB as PIL decoded the fixture (a gray file: three equal channels)."""
    global _pixels
    if _pixels is None:
        _pixels = dict(np.load(os.path.join(DIR, "pixels.npz")))
    a = _pixels[name]
    return a if a.ndim == 3 else np.repeat(a[:, :, None], 3, axis=2)


def info_struct(hs):
    info = hs._lib.HsflowJpegInfo()
    info.struct_size = ctypes.sizeof(info)
    return info


def header(hs, blob):
    info = info_struct(hs)
    buf = np.frombuffer(blob, np.uint8)
    st = hs._lib.load().hsflow_jpeg_read_header(ctypes.c_void_p(buf.ctypes.data), buf.size, ctypes.byref(info))
    return st, info


def decode_host_raw(hs, blob, order=RGB, pad=0, shape=None):
    """hsflow_jpeg_decode_host into rows `pad` bytes longer than tight, the buffer 0xA5 before: (status, info, rows)."""
    L = hs._lib.load()
    buf = np.frombuffer(blob, np.uint8) if len(blob) else np.zeros(1, np.uint8)
    st, info = header(hs, blob)
    H, W = shape if shape else ((info.height, info.width) if st == OK else (8, 8))
    rows = np.full((H, 3 * W + pad), 0xA5, np.uint8)
    info = info_struct(hs)
    st = L.hsflow_jpeg_decode_host(ctypes.c_void_p(buf.ctypes.data), len(blob), order, ctypes.c_void_p(rows.ctypes.data), rows.strides[0], ctypes.byref(info))
    return st, info, rows


def scan_range(hs, blob):
    st, info = header(hs, blob)
    assert st == OK
    return int(info.scan_offset), int(info.scan_bytes)


def cut_scan(hs, blob, keep):
    """The file with only the first `keep` bytes of its entropy-coded segment, and EOI behind them."""
    off, _ = scan_range(hs, blob)
    return blob[:off + keep] + b"\xff\xd9"


def huffman_codes(blob, tc, th):
    """{symbol: (code, length)} of the DHT table (class tc, id th) of a file."""
    i = 2
    while i + 4 <= len(blob):
        assert blob[i] == 0xFF
        m, ln = blob[i + 1], (blob[i + 2] << 8) | blob[i + 3]
        if m == 0xC4:
            s, e = i + 4, i + 2 + ln
            while s < e:
                counts = blob[s + 1:s + 17]
                total = sum(counts)
                if blob[s] == (tc << 4 | th):
                    out, code, k = {}, 0, 0
                    for length in range(1, 17):
                        for _ in range(counts[length - 1]):
                            out[blob[s + 17 + k]] = (code, length)
                            code += 1
                            k += 1
                        code <<= 1
                    return out
                s += 17 + total
        if m == 0xDA:
            break
        i += 2 + ln
    raise AssertionError("no such table")


def run_past_63(hs, blob):
    """A one-block gray file (the 8x8 fixture's header) whose only block has DC 0, three ZRL (zigzag position 49) and
    then a coefficient behind a run of 15: position 64.  Padded with 1-bits to a whole byte."""
    off, _ = scan_range(hs, blob)
    dc, ac = huffman_codes(blob, 0, 0), huffman_codes(blob, 1, 0)
    bits = ""
    for code, length in (dc[0], ac[0xF0], ac[0xF0], ac[0xF0], ac[0xF1]):
        bits += format(code, "0%db" % length)
    bits += "0"
    bits += "1" * (-len(bits) % 8)
    scan = bytes(int(bits[i:i + 8], 2) for i in range(0, len(bits), 8)).replace(b"\xff", b"\xff\x00")
    return blob[:off] + scan + b"\xff\xd9"
