"""CPU checks of the linking rule (csrc/hs_link_rule.h through hsflow_link_regions_host and hsflow_link_tracks_host): the
host form is held to the NumPy restatement of tests/link_ref.py byte for byte, and to closed forms that need no rule.  No
GPU work here."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import link_ref as R
from conftest import ROOT

F = np.float32
FILL = 0xA5
OK, E_ARG, E_SIZE = 0, 1, 2


def ptr(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


def padded(a, pad, fill):
    whole = np.full((a.shape[0], a.shape[1] + pad), fill, a.dtype)
    whole[:, :a.shape[1]] = a
    return whole[:, :a.shape[1]]


def host_link(hs, A, B, u, v, cap_a, cap_b, link_capacity, pad=0, ask=(True, True, True, True)):
    """hsflow_link_regions_host on planes whose rows are `pad` elements longer than the width: the bytes of (links written,
    side_a, side_b, result), None for what was not asked for, after checking that nothing was written behind an array."""
    H, W = A.shape
    aa, bb = padded(A, pad, 77), padded(B, (pad + 1) % 3, 78)
    uu, vv = padded(u, pad, F(7.0)), padded(v, pad, F(-3.0))
    lp = hs.make_link_params(cap_a, cap_b)
    links = np.full((link_capacity + 2) * 16, FILL, np.uint8) if ask[0] else None
    sa = np.full((cap_a + 1) * 32, FILL, np.uint8) if ask[1] else None
    sb = np.full((cap_b + 1) * 32, FILL, np.uint8) if ask[2] else None
    res = np.full(64 + 16, FILL, np.uint8) if ask[3] else None
    st = hs._lib.load().hsflow_link_regions_host(ptr(aa), aa.strides[0], ptr(bb), bb.strides[0], ptr(uu), ptr(vv), uu.strides[0], W, H, ctypes.byref(lp),
                                                  ptr(links), link_capacity, ptr(sa), ptr(sb), ctypes.cast(ptr(res), ctypes.POINTER(hs.HsflowLinkResult)))
    assert st == OK, hs._lib.load().hsflow_last_error(None)
    out = [None, None, None, None]
    if ask[3]:
        assert (res[64:] == FILL).all()
        out[3] = res[:64].tobytes()
    if ask[1]:
        assert (sa[cap_a * 32:] == FILL).all()
        out[1] = sa[:cap_a * 32].tobytes()
    if ask[2]:
        assert (sb[cap_b * 32:] == FILL).all()
        out[2] = sb[:cap_b * 32].tobytes()
    if ask[0]:
        n = len(R.link(A, B, u, v, cap_a, cap_b, link_capacity)[0])       # (the restatement's n_written: the header may be absent)
        assert (links[n:] == FILL).all()
        out[0] = links[:n].tobytes()
    return out


def header(hs, raw):
    return hs.HsflowLinkResult.from_buffer_copy(raw).as_dict()


# ---- H1. version, structs, defaults, symbols -------------------------------------------------------------------------------

def test_version_structs_defaults(hs):
    L = hs._lib.load()
    assert L.hsflow_version() >= 25
    text = open(os.path.join(ROOT, "include", "hsflow.h")).read()
    assert int(re.search(r"#define HSFLOW_VERSION_MINOR (\d+)", text).group(1)) >= 25
    assert ctypes.sizeof(hs.HsflowLinkParams) == 16 and ctypes.sizeof(hs.HsflowLinkRecord) == 16
    assert ctypes.sizeof(hs.HsflowLinkSide) == 32 and ctypes.sizeof(hs.HsflowLinkResult) == 64
    lp = hs.HsflowLinkParams()
    L.hsflow_default_link_params(ctypes.byref(lp))
    L.hsflow_default_link_params(None)
    assert (lp.struct_size, lp.cap_a, lp.cap_b, lp.reserved) == (16, 64, 64, 0)
    assert "#define HSFLOW_LINK_MAX_CELLS (1u << 24)" in text and hs.LINK_MAX_CELLS == 1 << 24
    assert int(re.search(r"#define HSFLOW_LINK_FLAG_OVERFLOW (\d+)u", text).group(1)) == 1 == hs.LINK_FLAG_OVERFLOW


def test_every_symbol_is_declared(hs):
    text = open(os.path.join(ROOT, "include", "hsflow.h")).read()
    names = set(re.findall(r"^(?:int|void) (hsflow_(?:default_)?link\w*)\(", text, re.M))
    assert names == {"hsflow_default_link_params", "hsflow_link_regions_host", "hsflow_link_regions_planes_device", "hsflow_link_regions_batch_device",
                     "hsflow_link_regions_device", "hsflow_link_regions", "hsflow_link_tracks_host"}
    L = hs._lib.load()
    for n in names:
        assert n in hs._lib.PROTOTYPES, n
        assert getattr(L, n).argtypes is not None, n


# ---- H2. the host form against the restatement ----------------------------------------------------------------------------

@pytest.mark.parametrize("W,H", R.SHAPES)
def test_host_equals_restatement(hs, W, H):
    for k, case in enumerate(R.CASES):
        A, B, u, v, cap_a, cap_b = R.planes(case, W, H)
        n_all = R.link(A, B, u, v, cap_a, cap_b, 0)[4]["n_links"]
        for capacity in (0, max(n_all - 1, 0), n_all + 2):
            want = R.link(A, B, u, v, cap_a, cap_b, capacity)
            got = host_link(hs, A, B, u, v, cap_a, cap_b, capacity, pad=k % 3)
            tag = (case, W, H, capacity)
            assert got[3] == want[3], (tag, header(hs, got[3]), want[4])
            assert got[0] == want[0] and got[1] == want[1] and got[2] == want[2], tag
            assert want[4]["flags"] == (1 if capacity < n_all else 0)


def test_each_output_alone(hs):
    W, H = 67, 19
    A, B, u, v, cap_a, cap_b = R.planes(R.CASES[8], W, H)
    want = R.link(A, B, u, v, cap_a, cap_b, 40)
    for one in range(4):
        ask = tuple(k == one for k in range(4))
        got = host_link(hs, A, B, u, v, cap_a, cap_b, 40, ask=ask)
        assert got[one] == want[one] and all(g is None for k, g in enumerate(got) if k != one)


# ---- H3. closed forms -------------------------------------------------------------------------------------------------------

def test_zero_flow_on_the_same_plane_is_the_diagonal(hs):
    W, H = 130, 37
    A = R.labels_of("random60", W, H)
    z = np.zeros((H, W), F)
    res, links, sa, sb = hs.link_regions_host(A, A, z, z, link_capacity=64, params=hs.make_link_params(60, 60))
    area = np.bincount(A.ravel(), minlength=61)
    n = int((area[1:] > 0).sum())
    assert res.n_links == n == res.n_mutual and res.voted_px == int(area[1:].sum()) and res.gone_px == res.unmatched_px == res.over_a_px == 0
    got = hs.link_records_from(links, n)
    assert [(r.a, r.b, r.px) for r in got] == [(k, k, int(area[k])) for k in range(1, 61) if area[k]]
    for k in range(1, 61):
        for s in (sa[k - 1], sb[k - 1]):
            assert (s.px, s.best_px, s.best, s.n_links) == ((int(area[k]), int(area[k]), k, 1) if area[k] else (0, 0, 0, 0))


def test_rectangle_under_an_integer_flow(hs):
    W, H = 40, 30
    A = np.zeros((H, W), np.int32)
    A[0:10, 30:40] = 1                               # 10 x 10 in the top right corner; (3, -2) takes it out by 3 columns and 2 rows
    B = np.zeros((H, W), np.int32)
    B[0:8, 33:40] = 5                                # where what stays inside arrives
    u, v = np.full((H, W), 3, F), np.full((H, W), -2, F)
    res, links, sa, sb = hs.link_regions_host(A, B, u, v, link_capacity=4, params=hs.make_link_params(2, 6))
    inside = 7 * 8
    assert (res.n_links, res.n_written, res.flags, res.n_mutual) == (1, 1, 0, 1)
    assert (res.voted_px, res.gone_px, res.unmatched_px) == (inside, 100 - inside, 0)
    assert (links[0].a, links[0].b, links[0].px, links[0].reserved) == (1, 5, inside, 0)
    assert sa[0].as_dict() == dict(px=100, n_links=1, best=5, best_px=inside, gone_px=100 - inside, unmatched_px=0)
    assert sb[4].as_dict() == dict(px=inside, n_links=1, best=1, best_px=inside, gone_px=0, unmatched_px=0)
    assert sa[1].as_dict() == dict(px=0, n_links=0, best=0, best_px=0, gone_px=0, unmatched_px=0)


def test_half_pixel_flows_pin_the_tie(hs):
    """x + 0.5 + 0.5 lands on x + 1; x - 0.5 + 0.5 lands on x: the half goes up, as floor(x + u + 0.5) says.  (The
    neighbours of the halves are chosen so that fl(3 + u) is not the half itself: fp32 has 2.4e-7 between values there.)"""
    W, H = 8, 3
    A = np.zeros((H, W), np.int32)
    A[1, 3] = 1
    B = np.arange(1, W * H + 1, dtype=np.int32).reshape(H, W)
    for du, dv, qx, qy in ((0.5, 0.0, 4, 1), (-0.5, 0.0, 3, 1), (0.0, 0.5, 3, 2), (0.0, -0.5, 3, 1), (-0.5000002, 0.0, 2, 1), (0.4999998, 0.0, 3, 1),
                           (1.5, -1.5, 5, 0), (-3.5, 0.0, 0, 1), (-3.5000002, 0.0, None, None), (4.5, 0.0, None, None), (4.4999995, 0.0, 7, 1)):
        u, v = np.full((H, W), du, F), np.full((H, W), dv, F)
        res, links, _, _ = hs.link_regions_host(A, B, u, v, link_capacity=2, params=hs.make_link_params(1, W * H), side_a=False, side_b=False)
        if qx is None:
            assert (res.n_links, res.gone_px) == (0, 1), (du, dv)
        else:
            assert (res.n_links, links[0].b, links[0].px) == (1, qy * W + qx + 1, 1), (du, dv)


def test_unknown_flow_is_gone(hs):
    W, H = 6, 4
    A = np.ones((H, W), np.int32)
    u, v = np.zeros((H, W), F), np.zeros((H, W), F)
    u[0, 0], v[1, 1], u[2, 2], v[3, 3], u[0, 5] = np.nan, np.nan, 1e10, -1e10, np.inf
    res, _, sa, _ = hs.link_regions_host(A, A, u, v, links=False, params=hs.make_link_params(1, 1))
    assert (res.gone_px, res.voted_px, sa[0].gone_px, sa[0].px, sa[0].best_px) == (5, W * H - 5, 5, W * H, W * H - 5)


def test_split_and_merge(hs):
    W, H = 20, 6
    one, halves = R.labels_of("one", W, H), R.labels_of("halves", W, H)
    z = np.zeros((H, W), F)
    res, links, sa, sb = hs.link_regions_host(one, halves, z, z, params=hs.make_link_params(2, 2), link_capacity=4)
    assert res.n_links == 2 and sa[0].n_links == 2 and sa[0].best == 1 and sa[0].best_px == 60 and res.n_mutual == 1      # the tie goes to the smaller b
    assert (sb[0].best, sb[1].best, sb[0].n_links, sb[1].n_links) == (1, 1, 1, 1)
    res, links, sa, sb = hs.link_regions_host(halves, one, z, z, params=hs.make_link_params(2, 2), link_capacity=4)
    assert res.n_links == 2 and sb[0].n_links == 2 and sb[0].best == 1 and res.n_mutual == 1 and (sa[0].best, sa[1].best) == (1, 1)
    assert [(r.a, r.b, r.px) for r in hs.link_records_from(links, 2)] == [(1, 1, 60), (2, 1, 60)]


def test_background_and_labels_above_the_caps(hs):
    W, H = 10, 2
    A = np.array([[-5, 0, 1, 2, 3, 4, 1, 2, 3, 4], [0] * 10], np.int32)
    B = np.array([[1, 2, 3, 4, 0, -1, 3, 2, 1, 0], [0] * 10], np.int32)
    z = np.zeros((H, W), F)
    res, links, sa, sb = hs.link_regions_host(A, B, z, z, params=hs.make_link_params(3, 2), link_capacity=8)
    # a = 4 twice: over_a; a = 1 -> b = 3 (above cap_b: unmatched), a = 1 -> b = 3 again; a = 2 -> 4 (unmatched), 2 -> 2; a = 3 -> 0, 3 -> 1
    assert (res.over_a_px, res.unmatched_px, res.voted_px, res.gone_px) == (2, 4, 2, 0)
    assert [(r.a, r.b, r.px) for r in hs.link_records_from(links, res.n_written)] == [(2, 2, 1), (3, 1, 1)]
    assert [s.unmatched_px for s in sa] == [2, 1, 1] and [s.px for s in sa] == [2, 2, 2] and [s.px for s in sb] == [1, 1]


# ---- H4. argument errors -----------------------------------------------------------------------------------------------------

def test_argument_errors(hs):
    L = hs._lib.load()
    W, H = 8, 4
    A, B = np.ones((H, W), np.int32), np.ones((H, W), np.int32)
    u, v = np.zeros((H, W), F), np.zeros((H, W), F)
    links, sa, sb = np.zeros(16 * 8 + 8, np.uint8), np.zeros(32 * 4 + 8, np.uint8), np.zeros(32 * 4 + 8, np.uint8)
    res = hs.HsflowLinkResult()
    good = hs.make_link_params(4, 4)

    def call(lp=good, a=A, b=B, uu=u, vv=v, sa_=4 * W, sb_=4 * W, fs=4 * W, w=W, h=H, k=ptr(links), cap=8, pa=ptr(sa), pb=ptr(sb), r=ctypes.pointer(res)):
        return L.hsflow_link_regions_host(a if isinstance(a, ctypes.c_void_p) or a is None else ptr(a), sa_, b if isinstance(b, ctypes.c_void_p) or b is None else ptr(b),
                                          sb_, uu if isinstance(uu, ctypes.c_void_p) or uu is None else ptr(uu), ptr(vv) if vv is not None else None, fs, w, h,
                                          ctypes.byref(lp) if lp is not None else None, k, cap, pa, pb, r)

    def off(a, n):
        return ctypes.c_void_p(a.ctypes.data + n)

    assert call() == OK
    bad = hs.make_link_params(4, 4); bad.struct_size = 12
    res1 = hs.make_link_params(4, 4); res1.reserved = 1
    for lp in (None, bad, res1, hs.make_link_params(0, 4), hs.make_link_params(4, 0)):
        assert call(lp=lp) == E_ARG
    assert call(a=None) == E_ARG and call(b=None) == E_ARG and call(uu=None) == E_ARG and call(vv=None) == E_ARG
    assert call(a=off(np.ones((H + 1, W), np.int32), 2)) == E_ARG and call(uu=off(np.zeros((H + 1, W), F), 1)) == E_ARG      # misaligned planes
    assert call(k=off(links, 4)) == E_ARG and call(pa=off(sa, 4)) == E_ARG and call(pb=off(sb, 2)) == E_ARG                     # misaligned records
    assert call(r=ctypes.cast(off(sa, 4), ctypes.POINTER(hs.HsflowLinkResult))) == E_ARG
    assert call(k=None, pa=None, pb=None, r=None) == E_ARG                                                                     # nothing asked for
    assert call(cap=0, pa=None, pb=None, r=None) == E_ARG and call(cap=0, pa=None, pb=None) == OK                               # a link array of no records is no output
    assert call(k=ptr(A)) == E_ARG and call(pa=ptr(u)) == E_ARG and call(pa=ptr(sb)) == E_ARG                                   # overlaps
    assert call(w=0) == E_SIZE and call(h=-1) == E_SIZE and call(w=16385) == E_SIZE
    assert call(sa_=4 * W - 4) == E_SIZE and call(sb_=4 * W + 2) == E_SIZE and call(fs=4 * W - 4) == E_SIZE
    assert call(lp=hs.make_link_params((1 << 30) + 1, 1), k=None, pa=None, pb=None) == E_SIZE
    assert call(lp=hs.make_link_params(4097, 4096), k=None, pa=None, pb=None) == E_SIZE
    assert call(lp=hs.make_link_params(1 << 16, 1 << 16), k=None, pa=None, pb=None) == E_SIZE                                   # (the product is formed in 64 bits)
    assert call(cap=(1 << 24) + 1, k=None) == E_SIZE
    assert call(lp=hs.make_link_params(4096, 4096), k=None, pa=None, pb=None) == OK and res.n_links == 1                         # the limit itself


# ---- H5. tracks --------------------------------------------------------------------------------------------------------------

def sides(hs, cap, rows):
    """A ctypes array of `cap` sides from {label: (px, best, best_px)}."""
    arr = (hs.HsflowLinkSide * cap)()
    for k, (px, best, best_px) in rows.items():
        arr[k - 1].px, arr[k - 1].best, arr[k - 1].best_px = px, best, best_px
    return arr


def test_tracks_continue_split_merge(hs):
    cap = 4
    # step 0: 1 -> 1 (continue); 2 splits into 2 (70 %) and 3 (30 %); step 1: 1 and 2 merge into 1 (2 sends more), 3 -> 2
    a0 = sides(hs, cap, {1: (100, 1, 100), 2: (100, 2, 70)})
    b0 = sides(hs, cap, {1: (100, 1, 100), 2: (70, 2, 70), 3: (30, 2, 30)})
    a1 = sides(hs, cap, {1: (100, 1, 100), 2: (120, 1, 120), 3: (30, 2, 30)})
    b1 = sides(hs, cap, {1: (220, 2, 120), 2: (30, 3, 30)})
    ids, n = hs.link_tracks([a0, a1], [b0, b1], [2, 3, 2], cap, min_share_256=128)
    assert ids.tolist() == [[1, 2, 0, 0], [1, 2, 3, 0], [2, 3, 0, 0]] and n == 3
    # the larger share keeps the id only if mutual: let region 2 of frame 1 prefer another sender
    b0x = sides(hs, cap, {1: (100, 1, 100), 2: (170, 1, 100), 3: (30, 2, 30)})
    ids, n = hs.link_tracks([a0], [b0x], [2, 3], cap, min_share_256=0)
    assert ids.tolist() == [[1, 2, 0, 0], [1, 3, 4, 0]] and n == 4


def test_tracks_share_threshold_and_caps(hs):
    cap = 2
    a0 = sides(hs, cap, {1: (100, 1, 50)})
    b0 = sides(hs, cap, {1: (50, 1, 50)})
    assert hs.link_tracks([a0], [b0], [1, 1], cap, min_share_256=128)[0].tolist() == [[1, 0], [1, 0]]       # 50 * 256 == 128 * 100: equality continues
    assert hs.link_tracks([a0], [b0], [1, 1], cap, min_share_256=129)[0].tolist() == [[1, 0], [2, 0]]
    a0 = sides(hs, cap, {1: (99, 1, 50)})
    assert hs.link_tracks([a0], [b0], [1, 1], cap, min_share_256=129)[0].tolist() == [[1, 0], [1, 0]]       # 50 * 256 = 12800 >= 129 * 99 = 12771
    ids, n = hs.link_tracks([a0], [b0], [7, 9], cap, min_share_256=0)                                        # n_regions above cap
    assert ids.tolist() == [[1, 2], [1, 3]] and n == 3
    ids, n = hs.link_tracks([], [], [1], cap)
    assert ids.tolist() == [[1, 0]] and n == 1
    L = hs._lib.load()
    ids = (ctypes.c_uint32 * 4)()
    cnt = (ctypes.c_uint32 * 2)(1, 1)
    pa, pb = (ctypes.c_void_p * 1)(ctypes.addressof(a0)), (ctypes.c_void_p * 1)(ctypes.addressof(b0))
    nul = (ctypes.c_void_p * 1)(None)
    assert L.hsflow_link_tracks_host(pa, pb, cnt, 1, cap, 128, ids, None) == OK
    assert L.hsflow_link_tracks_host(None, pb, cnt, 1, cap, 128, ids, None) == E_ARG and L.hsflow_link_tracks_host(pa, nul, cnt, 1, cap, 128, ids, None) == E_ARG
    assert L.hsflow_link_tracks_host(pa, pb, None, 1, cap, 128, ids, None) == E_ARG and L.hsflow_link_tracks_host(pa, pb, cnt, 1, cap, 128, None, None) == E_ARG
    assert L.hsflow_link_tracks_host(pa, pb, cnt, -1, cap, 128, ids, None) == E_ARG and L.hsflow_link_tracks_host(pa, pb, cnt, 1, 0, 128, ids, None) == E_ARG
    assert L.hsflow_link_tracks_host(pa, pb, cnt, 1, cap, 257, ids, None) == E_ARG and L.hsflow_link_tracks_host(pa, pb, cnt, 1, (1 << 30) + 1, 128, ids, None) == E_SIZE


# ---- H6. the rule under the sanitizers ------------------------------------------------------------------------------------

def test_rule_under_address_and_ub_sanitizers(tmp_path):
    """tests/link_host_san.cpp includes the rule header alone and links label planes with extreme flows in buffers that are
    exactly as large as the rule may touch; built with -fsanitize=address,undefined and run as a child process."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "link_host_san")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                        "-I", os.path.join(ROOT, "opticalflowhs_amd", "csrc"), os.path.join(ROOT, "tests", "link_host_san.cpp"), "-o", exe],
                       capture_output=True, text=True)
    if r.returncode != 0 and re.search(r"cannot find.*(asan|ubsan)|unsupported option|libasan|libubsan|libclang_rt", r.stderr):
        pytest.skip("the compiler has no sanitizer runtime")
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "link rule: ok" in r.stdout
