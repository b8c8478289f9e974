"""The one place that compiles host harness code (tests/hostkernel/*.cpp: the product's device headers built for the host), and the array helpers
the bindings and the test modules share.  TEST HARNESS ONLY."""
import ctypes as C
import os
import subprocess

import numpy as np

TESTS = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(TESTS, "hostkernel")
ROOT = os.path.dirname(TESTS)

# the lane code's results depend on these: no contraction, no fast math, the fma and vector instructions the harness was written against
BASE = ("g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-mavx2")
UBSAN = ("-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-g")


def command(src, flags=(), shared=True):
    """the compiler's command line of a target, without its output and its dependency file"""
    return list(BASE) + (["-fPIC", "-shared"] if shared else []) + list(flags) + [os.path.join(DIR, src)]


def dependencies(out):
    """the files the compiler read for `out` (its <out>.d, make syntax; paths without blanks), or None without one"""
    try:
        with open(out + ".d") as f:
            return f.read().replace("\\\n", " ").split(": ", 1)[1].split()
    except (OSError, IndexError):
        return None


def stale(out, owner):
    deps = dependencies(out)
    if deps is None or not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    return any(not os.path.exists(d) or os.path.getmtime(d) > t for d in deps + [os.path.abspath(__file__), owner])


def build(owner, src, out, flags=(), shared=True):
    """Compile src to out (both relative to tests/hostkernel, or absolute) unless out is up to date: a shared library, or an executable.
    owner: the file that holds the target's flags.  Up to date: out and out.d exist and nothing out.d names, nor this file, nor owner, is newer than
    out.  Both files appear atomically, the dependencies first: parallel test workers never load a half-written library, and a build interrupted
    between the two is stale."""
    out = os.path.join(DIR, out)
    if stale(out, owner):
        tmp, tmp_d = out + ".%d.tmp" % os.getpid(), out + ".d.%d.tmp" % os.getpid()
        subprocess.check_call(command(src, flags, shared) + ["-MMD", "-MF", tmp_d, "-o", tmp])
        os.replace(tmp_d, out + ".d")
        os.replace(tmp, out)
    return out


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _f32(a, shape):
    a = np.ascontiguousarray(a, np.float32)
    assert a.shape == shape, (a.shape, shape)
    return a


def bits(a):
    """the uint32 view of an array of float32 (converted to it if need be)"""
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    """bit for bit: a NaN equals only the same NaN, 0 does not equal -0"""
    return np.array_equal(bits(a), bits(b))
