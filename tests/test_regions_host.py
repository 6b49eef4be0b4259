"""CPU checks of the labelling rule (csrc/hs_regions_rule.h through hsflow_regions_host): the host form is held to the
breadth-first restatement of tests/regions_ref.py exactly -- labels, records and headers as integers -- and, where SciPy
is there, its partition to scipy.ndimage.label's.  No GPU work here."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import regions_ref as R
from conftest import ROOT

F = np.float32
FILL = 0xA5
RECORD_FIELDS = ("root", "area", "x0", "y0", "x1", "y1", "sum_x", "sum_y", "n_flow", "reserved0", "sum_qu", "sum_qv", "reserved1")
RESULT_FIELDS = ("n_regions", "n_written", "n_dropped", "flags", "fg_px", "dropped_px", "unknown_flow_px", "largest_area", "largest_label")
CASES = [c[0] for c in R.cases()]


def ptr(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


def padded(a, pad, fill):
    whole = np.full((a.shape[0], a.shape[1] + pad), fill, a.dtype)
    whole[:, :a.shape[1]] = a
    return whole[:, :a.shape[1]], whole


def record_dict(r):
    return {k: int(getattr(r, k)) for k in RECORD_FIELDS}


def result_dict(r):
    d = {k: int(getattr(r, k)) for k in RESULT_FIELDS}
    assert list(r.reserved) == [0, 0]
    return d


def host_label(hs, mask, u, v, rp, W, H, capacity, with_records=True, pad=0):
    """hsflow_regions_host on planes whose rows are `pad` elements longer than the width: (labels, records as dicts, result as
    dict), after checking that nothing beyond a row's width and no record from n_written on was written."""
    mm = padded(mask, pad, 0)[0] if mask is not None else None
    uu = padded(u, pad, F(7.0))[0] if u is not None else None
    vv = padded(v, pad, F(-3.0))[0] if v is not None else None
    labels, lw = padded(np.zeros((H, W), np.int32), pad, 0x5A5A5A5A)
    recs = np.full((capacity + 2) * 64, FILL, np.uint8) if with_records else None
    res = hs.HsflowRegionsResult()
    st = hs._lib.load().hsflow_regions_host(ptr(mm), mm.strides[0] if mm is not None else 0, ptr(uu), ptr(vv), uu.strides[0] if uu is not None else 0, W, H,
                                             ctypes.byref(rp), ptr(labels), labels.strides[0], ptr(recs), capacity, ctypes.byref(res))
    assert st == 0, hs._lib.load().hsflow_last_error(None)
    assert (lw[:, W:] == 0x5A5A5A5A).all()
    out = []
    if with_records:
        assert (recs[res.n_written * 64:] == FILL).all()
        out = [record_dict(hs.HsflowRegionsRecord.from_buffer_copy(recs[k * 64:(k + 1) * 64].tobytes())) for k in range(res.n_written)]
    return labels.copy(), out, result_dict(res)


# ---- H1. version, structs, defaults, symbols -------------------------------------------------------------------------------

def test_version_structs_defaults(hs):
    L = hs._lib.load()
    assert L.hsflow_version() >= 24
    text = open(os.path.join(ROOT, "include", "hsflow.h")).read()
    assert int(re.search(r"#define HSFLOW_VERSION_MINOR (\d+)", text).group(1)) >= 24
    assert ctypes.sizeof(hs.HsflowRegionsParams) == 32 and ctypes.sizeof(hs.HsflowRegionsRecord) == 64 and ctypes.sizeof(hs.HsflowRegionsResult) == 64
    rp = hs.HsflowRegionsParams()
    L.hsflow_default_regions_params(ctypes.byref(rp))
    L.hsflow_default_regions_params(None)
    assert (rp.struct_size, rp.connectivity, rp.fg_lo, rp.fg_hi, rp.min_area, rp.join_px, list(rp.reserved)) == (32, 8, 1, 255, 1, 0.0, [0, 0])
    assert int(re.search(r"#define HSFLOW_REGIONS_MAX_SIDE (\d+)", text).group(1)) == 16384 == hs.REGIONS_MAX_SIDE
    assert int(re.search(r"#define HSFLOW_REGIONS_FLAG_OVERFLOW (\d+)u", text).group(1)) == 1 == hs.REGIONS_FLAG_OVERFLOW


def test_every_symbol_is_declared(hs):
    text = open(os.path.join(ROOT, "include", "hsflow.h")).read()
    names = set(re.findall(r"^(?:int|void) (hsflow_(?:default_)?regions\w*)\(", text, re.M))
    assert names == {"hsflow_default_regions_params", "hsflow_regions_host", "hsflow_regions_planes_device", "hsflow_regions_batch_device", "hsflow_regions_device",
                     "hsflow_regions"}
    L = hs._lib.load()
    for n in names:
        assert n in hs._lib.PROTOTYPES, n
        assert getattr(L, n).argtypes is not None, n


# ---- H2. the host form against the restatement ----------------------------------------------------------------------------

@pytest.mark.parametrize("W,H", R.SHAPES)
def test_host_equals_restatement(hs, W, H):
    for case in CASES:
        mask, u, v, join = R.planes(case, W, H)
        for conn in (4, 8):
            for min_area in (1, 2, 5):
                n_all = R.want(case, W, H, conn, min_area, 0)["result"]["n_regions"]
                for capacity, with_records in ((0, False), (3, True), (n_all + 2, True)):
                    want = R.want(case, W, H, conn, min_area, capacity)
                    rp = hs.make_regions_params(connectivity=conn, min_area=min_area, join_px=join)
                    labels, recs, res = host_label(hs, mask, u, v, rp, W, H, capacity, with_records, pad=(conn + min_area) % 4)
                    tag = (case, W, H, conn, min_area, capacity)
                    assert res == want["result"], tag
                    assert np.array_equal(labels, want["labels"]), tag
                    if with_records:
                        assert recs == want["records"], tag


def test_foreground_range_and_join0_with_flow(hs):
    """fg_lo .. fg_hi select the bytes; flow planes under join_px 0 change the sums and nothing else."""
    W, H = 96, 64
    mask = R.mask_of("random59", W, H)
    u, v = R.flow_of("sprinkled", W, H)
    for lo, hi in ((1, 255), (0, 0), (100, 180), (255, 255), (0, 255)):
        rp = hs.make_regions_params(connectivity=4, fg=(lo, hi))
        want = R.label(mask, u, v, 4, 1, 0.0, 5000, fg=(lo, hi))
        labels, recs, res = host_label(hs, mask, u, v, rp, W, H, 5000)
        assert res == want["result"] and np.array_equal(labels, want["labels"]) and recs == want["records"], (lo, hi)
        plain = host_label(hs, mask, None, None, rp, W, H, 5000)
        assert np.array_equal(plain[0], labels) and plain[2]["unknown_flow_px"] == 0
        assert [dict(r, n_flow=0, sum_qu=0, sum_qv=0) for r in recs] == plain[1]


def test_partition_equals_scipy(hs):
    ndi = pytest.importorskip("scipy.ndimage")
    for W, H in R.SHAPES:
        for name in R.MASKS:
            mask = R.mask_of(name, W, H)
            for conn in (4, 8):
                labels, _, res = host_label(hs, mask, None, None, hs.make_regions_params(connectivity=conn), W, H, 0, False)
                theirs, n = ndi.label(mask != 0, structure=np.ones((3, 3), int) if conn == 8 else None)
                assert n == res["n_regions"] and R.same_partition(labels, theirs), (name, W, H, conn)


# ---- H3. every documented refusal -----------------------------------------------------------------------------------------

def test_every_documented_error(hs):
    L = hs._lib.load()
    E_ARG, E_SIZE = hs._lib.E_ARG, hs._lib.E_SIZE
    W, H = 20, 6
    mask = np.full((H, W), 255, np.uint8)
    u = np.zeros((H, W), F)
    v = np.zeros((H, W), F)
    labels = np.zeros((H, W), np.int32)
    recs = np.zeros(4 * 64 + 8, np.uint8)
    recs = recs[(-recs.ctypes.data) % 8:][:4 * 64]
    res = hs.HsflowRegionsResult()

    def call(rp=None, mask=mask, ms=None, u=None, v=None, fs=None, W=W, H=H, labels=labels, ls=None, recs=recs, cap=4, res=res, rp_null=False):
        rp = rp if rp is not None else hs.make_regions_params()
        return L.hsflow_regions_host(ptr(mask) if not isinstance(mask, int) else ctypes.c_void_p(mask), ms if ms is not None else W,
                                     ptr(u) if not isinstance(u, int) else ctypes.c_void_p(u), ptr(v) if not isinstance(v, int) else ctypes.c_void_p(v),
                                     fs if fs is not None else 4 * W, W, H, None if rp_null else ctypes.byref(rp),
                                     ptr(labels) if not isinstance(labels, int) else ctypes.c_void_p(labels), ls if ls is not None else 4 * W,
                                     ptr(recs) if not isinstance(recs, int) else ctypes.c_void_p(recs), cap, ctypes.byref(res) if res is not None else None)

    assert call() == 0
    assert call(u=u, v=v, rp=hs.make_regions_params(join_px=1.0)) == 0

    def params(**kw):
        rp = hs.make_regions_params()
        for k, x in kw.items():
            setattr(rp, k, x)
        return rp

    assert call(rp_null=True) == E_ARG
    assert call(rp=params(struct_size=28)) == E_ARG
    rp = hs.make_regions_params()
    rp.reserved[1] = 1
    assert call(rp=rp) == E_ARG
    for conn in (3, 0, 6, -4):
        assert call(rp=params(connectivity=conn)) == E_ARG
    assert call(rp=params(fg_lo=9, fg_hi=8)) == E_ARG
    assert call(rp=params(fg_lo=-1)) == E_ARG
    assert call(rp=params(fg_hi=256)) == E_ARG
    assert call(rp=params(min_area=0)) == E_ARG
    for bad in (float("nan"), -0.5, float("inf"), 3e38, 1e-30):
        assert call(rp=params(join_px=bad), u=u, v=v) == E_ARG, bad
    assert call(rp=params(join_px=1.0)) == E_ARG                       # join without flow
    assert call(u=u) == E_ARG and call(v=v) == E_ARG                    # one flow plane without the other
    assert call(u=u.ctypes.data + 2, v=v) == E_ARG                      # a flow plane that is not 4-byte aligned
    assert call(labels=labels.ctypes.data + 2) == E_ARG
    assert call(recs=recs.ctypes.data + 4) == E_ARG
    assert call(labels=None, recs=None, res=None) == E_ARG              # nothing asked for
    assert call(labels=None, recs=None) == 0 and call(labels=None, res=None) == 0 and call(recs=None, res=None) == 0
    # overlap: an output on an input, two outputs on one another
    assert call(labels=mask.ctypes.data // 4 * 4) == E_ARG
    assert call(u=u, v=labels.view(F)) == E_ARG
    assert call(recs=labels.ctypes.data // 8 * 8 + 8) == E_ARG
    # strides and sizes
    assert call(ms=W - 1) == E_SIZE
    assert call(u=u, v=v, fs=4 * W - 4) == E_SIZE and call(u=u, v=v, fs=4 * W + 2) == E_SIZE
    assert call(ls=4 * W - 4) == E_SIZE and call(ls=4 * W + 2) == E_SIZE
    assert call(W=0) == E_SIZE and call(H=0) == E_SIZE and call(W=-3) == E_SIZE
    assert call(W=16385, H=1, mask=None, labels=None, recs=None) == E_SIZE and call(W=1, H=16385, mask=None, labels=None, recs=None) == E_SIZE
    assert call(cap=(1 << 30) + 1, recs=None) == E_SIZE
    assert L.hsflow_last_error(None)


def test_largest_side_is_accepted(hs):
    """A side of 16384 is inside the rule: one row, a mask of runs."""
    W = 16384
    mask = np.zeros((1, W), np.uint8)
    mask[0, 5:W - 3] = 1
    mask[0, 9000] = 0
    labels, recs, res = host_label(hs, mask, None, None, hs.make_regions_params(connectivity=4), W, 1, 4)
    assert res["n_regions"] == 2 and [r["area"] for r in recs] == [8995, W - 3 - 9001] and recs[1]["x1"] == W - 4
    assert recs[0]["sum_x"] == sum(range(5, 9000)) and res["largest_label"] == 1


# ---- H4. the rule under the sanitizers ------------------------------------------------------------------------------------

def test_rule_under_address_and_ub_sanitizers(tmp_path):
    """tests/regions_host_san.cpp includes the rule header alone and labels the patterns at (260, 37) and (1, 40) in buffers
    that are exactly as large as the rule may touch; built with -fsanitize=address,undefined and run as a child process."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "regions_host_san")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                        "-I", os.path.join(ROOT, "opticalflowhs_amd", "csrc"), os.path.join(ROOT, "tests", "regions_host_san.cpp"), "-o", exe],
                       capture_output=True, text=True)
    if r.returncode != 0 and re.search(r"cannot find.*(asan|ubsan)|unsupported option|libasan|libubsan|libclang_rt", r.stderr):
        pytest.skip("the compiler has no sanitizer runtime")
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "regions rule: ok" in r.stdout
