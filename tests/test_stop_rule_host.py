"""CPU check of the ITER|EPS witness rule (csrc/hs_stop_rule.h): for every epsilon and every launch length the planner
can choose, either the host refuses the witness pass, or the threshold it hands to the kernels survives the kernels'
integer exponent step -- the stepped bits ARE thr * 4^(s+1), finite and positive -- and thr >= epsilon, so that "change
>= stepped threshold" implies "Eps >= epsilon".  The header is compiled alone with g++; the kernels' step
(hs_kernels_strip.hip.h: float_as_int(eps_thr) + ((s + 1) << 24)) is restated here in numpy.  No device needed."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "opticalflowhs_amd", "csrc")
FLT_MAX = float(np.finfo(np.float32).max)
FLT_MIN = float(np.finfo(np.float32).tiny)


def max_fuse():
    m = re.search(r"constexpr\s+int\s+kMaxFuse\s*=\s*(\d+)\s*;", open(os.path.join(CSRC, "hs_context.hip.h")).read())
    assert m
    return int(m.group(1))


def kernel_step(thr_bits, s):
    """The bits of the threshold of sweep s of a launch, as the kernels form them (32-bit wrap-around included)."""
    return np.uint32((int(thr_bits) + ((s + 1) << 24)) & 0xFFFFFFFF)


def as_float(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


def epsilons():
    out = []
    for e in range(-1080, 1025):                           # every exponent of a double (denormal ones included) ...
        for m in (1.0, 1.25, 1.5, 1.9999999, 2.0 - 2.0 ** -52):  # ... a few mantissas, the last float and the last double under 2
            with np.errstate(over="ignore"):
                out.append(float(np.ldexp(m, e)))
    for e in range(-149, 128):                             # every float exponent: the float itself and doubles around it
        f = np.ldexp(np.float32(1.0), e)
        up = np.nextafter(f, np.float32(np.inf))
        out += [float(f), float(up), float(np.nextafter(np.float64(f), np.inf)), float(np.nextafter(np.float64(f), 0.0)),
                float(f) + (float(up) - float(f)) * 0.25, float(f) + (float(up) - float(f)) * 0.5]
    out += [0.0, -0.0, 5e-324, 1e-45, 1e-40, FLT_MIN, float(np.nextafter(np.float64(FLT_MIN), 0.0)), 1e-9, 1e-6, 0.5, 1.0, 1e30,
            FLT_MAX, float(np.nextafter(np.float64(FLT_MAX), np.inf)), 2.0 ** 126, 2.0 ** 127, 2.0 ** 128, 1e39, 1e300,
            float("inf"), -1.0, -1e-40, -FLT_MAX, -1e300, float("-inf"), float("nan"), -float("nan")]
    return out


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the stand-alone rule check"
    exe = str(tmp_path_factory.mktemp("stop_rule") / "stop_rule")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=undefined", "-fno-sanitize-recover=all",
                        "-static-libubsan", "-I", CSRC, os.path.join(ROOT, "tests", "stop_rule_main.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(eps_list, tmax):
        text = "".join("%016x\n" % struct.unpack("<Q", struct.pack("<d", e))[0] for e in eps_list)
        p = subprocess.run([exe, str(tmax)], input=text, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr
        rows = [ln.split() for ln in p.stdout.splitlines()]
        assert len(rows) == len(eps_list)
        return [(int(t, 16), [c == "1" for c in u]) for t, u in rows]
    return run


def test_every_epsilon_is_refused_or_scales_exactly(rule):
    tmax = max_fuse()
    eps = epsilons()
    rows = rule(eps, tmax)
    e = np.array(eps, np.float64)
    tb = np.array([r[0] for r in rows], np.uint32)
    usable = np.array([r[1] for r in rows], bool)            # [epsilon, T - 1]
    assert usable.shape == (len(eps), tmax)
    thr = tb.view(np.float32).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        for T in range(1, tmax + 1):
            ok = usable[:, T - 1]
            # refused for a reason: a NaN, or a threshold whose last step leaves the finite range -- not at random
            assert np.all(np.isnan(e[~ok]) | (thr[~ok] * 4.0 ** T > FLT_MAX)), T
            assert np.all(thr[ok] >= e[ok]), T               # (false for a NaN: a NaN must have been refused)
            for s in range(T):
                bits = ((tb[ok].astype(np.uint64) + ((s + 1) << 24)) & 0xFFFFFFFF).astype(np.uint32)   # the kernels' step
                got = bits.view(np.float32)
                want = np.ldexp(thr[ok], 2 * (s + 1))
                assert np.all(np.isfinite(got) & (got > 0)), (T, s)
                assert np.array_equal(got.astype(np.float64), want), (T, s)
                assert np.array_equal(bits, want.astype(np.float32).view(np.uint32)), (T, s)
    assert (~usable[~np.isnan(e)]).any() and usable.any()


def test_the_threshold_is_the_smallest_normal_float_at_or_above_epsilon(rule):
    eps = [e for e in epsilons() if e == e]
    for e, (tb, _) in zip(eps, rule(eps, 1)):
        thr = as_float(tb)
        if e > FLT_MAX:
            assert np.isposinf(thr), e
        elif e <= FLT_MIN:
            assert float(thr) == FLT_MIN, e
        else:
            assert float(thr) >= e and float(np.nextafter(thr, np.float32(0))) < e, (e, thr)


def test_what_is_refused_at_the_top_of_the_range(rule):
    """The cases of the solve path by name: every epsilon >= 2^127 is refused for every launch length (the parent's rule
    let them through: the stepped bits carry into the sign bit), 2^(127 - 2T) is the last power of two a launch of T sweeps
    takes, and the everyday range is never refused."""
    tmax = max_fuse()
    top = [2.0 ** 127, FLT_MAX, 1e39, float("inf")]
    for e, (tb, usable) in zip(top, rule(top, tmax)):
        assert not any(usable), e
        for s in range(tmax):                               # ... and what the kernels would have made of it
            assert not as_float(kernel_step(tb, s)) > 0, (e, s)
    edge = [2.0 ** (127 - 2 * T) for T in range(1, tmax + 1)]
    for T, (e, (tb, usable)) in enumerate(zip(edge, rule(edge, tmax)), 1):
        assert usable == [t <= T for t in range(1, tmax + 1)], (T, usable)
    daily = [1e-9, 1e-6, 1e-3, 0.5, 0.0, -1.0, 1e-40, 5e-324, FLT_MIN]
    for e, (tb, usable) in zip(daily, rule(daily, tmax)):
        assert all(usable), e
