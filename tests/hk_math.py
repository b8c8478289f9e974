"""ctypes binding of tests/hostkernel/libmath_host.so: the product's math layer (vr_math.h) built for the host behind the probe table of
vr_math_probe.h, a float64 libm reference for the accuracy tests, and the input sets the math tests share.  TEST HARNESS ONLY."""
import ctypes as C
import json
import os

import numpy as np

import hk_common

_lib = None
ACCURACY_JSON = os.path.join(hk_common.TESTS, "golden", "math_accuracy.json")

# probe codes (volren_amd/csrc/vr_math_probe.h)
LOG, SIN, COS, TAN, ACOS, ATAN2, EXP, POW, ASIN = range(9)
HALF2FLOAT, RCP_EXACT = 15, 16
SINCOS_S, SINCOS_C, NEG_LOG_1M, LOG_UNIT, FLOOR2I, VOXEL_INDEX, ROUND_MIP, ROUND_MIP_Q, ROUND_HALF_EVEN = range(18, 27)
SCALE2, SANITIZE, MIN, MAX, CLAMP_LO, CLAMP_HI, HALF_RNE, HALF_DOWN, HALF_UP, MUL24, UNORM8 = range(27, 38)
FAST_NEG_LOG_1M, FAST_SIN, FAST_COS, FAST_UNORM8 = 100, 101, 102, 103          # vr_math_sweep only: the tolerance-mode forms
NAMES = {LOG: "log_", SIN: "sin_", COS: "cos_", TAN: "tan_", ACOS: "acos_", ATAN2: "atan2_", EXP: "exp_", POW: "pow_", ASIN: "asin_",
         SINCOS_S: "sincos_.s", SINCOS_C: "sincos_.c", NEG_LOG_1M: "neg_log_1m", LOG_UNIT: "log_unit_"}


TWO_PI_BITS = 0x40C90FDB          # float32(2 pi)
LIVE = " on [0, 2 pi]"            # suffix of the recorded entries of sincos_ on the angles the renderer forms


def build():
    return hk_common.build(__file__, "math_host.cpp", "libmath_host.so", ("-fopenmp",))


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        vp, ll, u = C.c_void_p, C.c_longlong, C.c_uint32
        L.hk_math_batch.argtypes = [C.c_int, vp, vp, vp, ll]
        L.hk_math_sweep.argtypes = [C.c_int, u, ll, u, vp]
        L.hk_math_accuracy.argtypes = [C.c_int, vp, vp, vp, u, ll, vp]
        _lib = L
    return _lib


def bits(a):
    """the uint32 view of a 4-byte array (float32 values, or integers carried as bit patterns).  Not hk_common.bits: integers keep their bits instead
    of being converted to float32, and the result is flat."""
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "f" and a.dtype.itemsize != 4:
        a = a.astype(np.float32)
    assert a.dtype.itemsize == 4, a.dtype
    return a.view(np.uint32).reshape(-1)


def f32(u):
    return np.ascontiguousarray(u, np.uint32).view(np.float32)


def _ptr(a):
    return a.ctypes.data if a is not None else None


def _operands(a, b):
    a = bits(a)
    if b is not None:
        b = bits(b)
        if b.size == 1 and a.size != 1:
            b = np.full(a.size, b[0], np.uint32)
        assert b.size == a.size
    return a, b


def batch(fn, a, b=None):
    """the host build's f(a, b): uint32 result bits"""
    a, b = _operands(a, b)
    out = np.empty(a.size, np.uint32)
    if lib().hk_math_batch(int(fn), _ptr(a), _ptr(b), _ptr(out), a.size) != 0:
        raise ValueError("no math probe %d" % fn)
    return out


def sweep(fn, first, count, b=0.0):
    out = np.empty(int(count), np.uint32)
    if lib().hk_math_sweep(int(fn), int(first) & 0xFFFFFFFF, int(count), int(bits(np.float32(b))[0]), _ptr(out)) != 0:
        raise ValueError("no math probe %d" % fn)
    return out


def _accuracy(fn, a, b, got, first, n):
    out = np.zeros(7, np.float64)
    if lib().hk_math_accuracy(int(fn), _ptr(a), _ptr(b), _ptr(got), int(first) & 0xFFFFFFFF, int(n), _ptr(out)) != 0:
        raise ValueError("no float64 reference for math probe %d" % fn)
    return {"max_ulp": float(out[0]), "worst": [int(out[1]), int(out[2])], "max_abs": float(out[3]), "worst_abs": [int(out[4]), int(out[5])], "points": int(out[6])}


def accuracy(fn, a, b=None, got=None):
    """Error against float64 libm over the part of (a, b) inside fn's specified domain; `got`: float32 results to judge instead of the host build's.
    max_ulp is in ulps of the correctly rounded float32 result, worst / worst_abs are the operands' bit patterns."""
    a, b = _operands(a, b)
    got = bits(got) if got is not None else None
    return _accuracy(fn, a, b, got, 0, a.size)


def accuracy_sweep(fn, first, count, got=None):
    return _accuracy(fn, None, None, bits(got) if got is not None else None, first, count)


def recorded():
    with open(ACCURACY_JSON) as f:
        return json.load(f)


def bound(ulps):
    """a recorded maximum rounded up to the next 0.05 ulp: the margin covers the float64 reference's own error and another host's libm"""
    return (np.floor(ulps / 0.05 + 1e-9) + 1.0) * 0.05


# ---- input sets ---------------------------------------------------------------------------------------------------------------------------
EDGE_MANTISSAS = np.array([0, 1, 2, 0x3FFFFF, 0x400000, 0x400001, 0x7FFFFE, 0x7FFFFF], np.uint32)


def lattice(n_mantissas, seed=11):
    """every exponent x both signs x n_mantissas mantissas (the eight edge ones and random ones): uint32 bit patterns"""
    rs = np.random.RandomState(seed)
    m = np.concatenate([EDGE_MANTISSAS, rs.randint(0, 1 << 23, n_mantissas - EDGE_MANTISSAS.size).astype(np.uint32)])
    e = np.arange(256, dtype=np.uint32) << 23
    pos = (e[:, None] | m[None, :]).reshape(-1)
    return np.concatenate([pos, pos | np.uint32(0x80000000)])


def _around(values):
    """each float32 value with its two neighbours"""
    v = np.asarray(values, np.float32)
    return bits(np.concatenate([np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf))]))


def specials():
    """+-0, +-smallest / largest denormal, +-FLT_MIN, +-1 and neighbours, +-FLT_MAX, +-inf, a quiet and a signalling-pattern NaN, and the functions' own
    thresholds +-1 ulp (sin_'s 8192, exp_'s two cut-offs, asin_'s 0.5 and 1e-4, atan_'s tan(pi/8) and tan(3pi/8), log_'s sqrt(1/2)): uint32 bit patterns"""
    pos = np.concatenate([
        np.array([0, 1, 0x007FFFFF, 0x00800000, 0x7F7FFFFF, 0x7F800000], np.uint32),
        _around([1.0, 8192.0, 88.72283905206835, 103.278929903431851103, 0.5, 1.0e-4, 0.4142135623730950, 2.414213562373095, 0.707106781186547524])])
    return np.concatenate([pos, pos | np.uint32(0x80000000), np.array([0x7FC00000, 0x7FA00000, 0xFFC00001], np.uint32)])


def cross(u):
    """the full cross product of a set with itself: (a, b)"""
    a, b = np.meshgrid(u, u, indexing="ij")
    return a.reshape(-1).copy(), b.reshape(-1).copy()


def unit_directions(n=1 << 21, seed=5):
    """(z, x) components of n unit directions -- what the environment lookup hands to atan2_ -- and of the axis-aligned ones with exact and negative zeros"""
    rs = np.random.RandomState(seed)
    v = rs.standard_normal((n, 3))
    v = (v / np.sqrt((v * v).sum(axis=1, keepdims=True))).astype(np.float32)
    ax = np.array([[x, y, z] for x in (-1.0, -0.0, 0.0, 1.0) for y in (-1.0, -0.0, 0.0, 1.0) for z in (-1.0, -0.0, 0.0, 1.0)], np.float32)
    ax = ax[(np.abs(ax).sum(axis=1) == 1.0)]
    v = np.concatenate([v, ax])
    return bits(v[:, 2].copy()), bits(v[:, 0].copy())


def pow_domains(seed=6):
    """pow_'s two live domains, as (x, y) bit patterns.  Tonemapper: x in [0, 1] and y = 1 / gamma -- the renderer takes any gamma, so every gamma from 0.25 to 8 in steps
    of 1/64 plus the usual 1, 1.8, 2.2, 2.4.  Denoiser: x = a clamped cosine in [0, 1] and y = the normal sigma, which vr_set_float keeps within [2^-60, 2^60]."""
    rs = np.random.RandomState(seed)
    x = np.concatenate([np.array([0.0, 1.0, np.nextafter(np.float32(1), np.float32(0)), 1e-45, 1.17549435e-38], np.float32),
                        rs.uniform(0, 1, 2043).astype(np.float32)])
    gam = np.concatenate([np.arange(16, 513, dtype=np.float32) / np.float32(64), np.array([1.0, 1.8, 2.2, 2.4], np.float32)])
    inv = (np.float32(1) / gam).astype(np.float32)
    sig = np.concatenate([np.ldexp(np.float32(1), np.arange(-60, 61)).astype(np.float32), np.exp(rs.uniform(np.log(2.0 ** -60), np.log(2.0 ** 60), 391)).astype(np.float32)])
    xa, ya = np.meshgrid(x, inv, indexing="ij")
    xb, yb = np.meshgrid(x, sig, indexing="ij")
    return (bits(np.concatenate([xa.reshape(-1), xb.reshape(-1)])), bits(np.concatenate([ya.reshape(-1), yb.reshape(-1)])))


def scale2_set(seed=8):
    """scale2(z, n): every n in [-300, 300] on a mantissa set over a few exponents (results from 0 through the denormals to inf): (z bits, n as bits)"""
    rs = np.random.RandomState(seed)
    m = np.concatenate([EDGE_MANTISSAS, rs.randint(0, 1 << 23, 56).astype(np.uint32)])
    e = np.array([0, 1, 2, 64, 126, 127, 128, 190, 253, 254, 255], np.uint32) << 23
    z = (e[:, None] | m[None, :]).reshape(-1)
    z = np.concatenate([z, z | np.uint32(0x80000000)])
    n = np.arange(-300, 301, dtype=np.int32)
    za, na = np.meshgrid(z, n.view(np.uint32), indexing="ij")
    return za.reshape(-1).copy(), na.reshape(-1).copy()


def draws():
    """every random draw xi = k 2^-24 of the renderer's generator"""
    return bits((np.arange(1 << 24, dtype=np.float32) / np.float32(1 << 24)))


def floored_lattice(n_mantissas=1 << 12):
    """floor() of every lattice value that is not NaN: what voxel_index is given"""
    x = f32(lattice(n_mantissas, seed=12))
    return bits(np.floor(x[~np.isnan(x)]))


_cases = None


def array_cases():
    """The (name, fn, a bits, b bits or None) comparisons that the host build and the device are both held to, beyond the unary sweeps."""
    global _cases
    if _cases is not None:
        return _cases
    rs = np.random.RandomState(9)
    sp = specials()
    sa, sb = cross(sp)
    c = []
    for fn in (ATAN2, POW, MIN, MAX, CLAMP_LO, CLAMP_HI):
        c.append(("specials", fn, sa, sb))
    n_all = np.arange(-300, 301, dtype=np.int32).view(np.uint32)
    za, na = np.meshgrid(sp, n_all, indexing="ij")
    c.append(("specials x n", SCALE2, za.reshape(-1).copy(), na.reshape(-1).copy()))
    c.append(("mantissas x n", SCALE2) + scale2_set())
    c.append(("unit directions", ATAN2) + unit_directions())
    c.append(("tonemapper and denoiser", POW) + pow_domains())
    fl = floored_lattice()
    for o in (-2, -1, 0, 1, 2):
        c.append(("floored lattice, o = %d" % o, VOXEL_INDEX, fl, np.full(fl.size, o, np.int32).view(np.uint32)))
    q = np.arange(13, dtype=np.int32)
    c.append(("q = 0..12", ROUND_MIP, bits(q.astype(np.float32) / np.float32(4)), None))
    c.append(("q = 0..12", ROUND_MIP_Q, q.view(np.uint32), None))
    quarters = (np.arange(-4096, 4097, dtype=np.float32) / np.float32(4))
    c.append(("quarters and neighbours", ROUND_HALF_EVEN, _around(quarters), None))
    edge = np.array([0, 1, 2, 255, 256, 4095, 4096, 4097, 65535, 65536, (1 << 24) - 1], np.uint64)
    ea, eb = np.meshgrid(edge, edge, indexing="ij")
    ra, rb = rs.randint(0, 1 << 24, 200000).astype(np.uint64), rs.randint(0, 1 << 24, 200000).astype(np.uint64)
    rb = np.where(ra * rb < (1 << 32), rb, ((1 << 32) - 1) // np.maximum(ra, 1))                  # random pairs, second factor cut so that the product fits
    ma, mb = np.concatenate([ea.reshape(-1), ra, ra]), np.concatenate([eb.reshape(-1), rb, rs.randint(0, 256, 200000).astype(np.uint64)])
    ok = (ma * mb < (1 << 32)) & (mb < (1 << 24))
    c.append(("domain edges and random pairs", MUL24, ma[ok].astype(np.uint32), mb[ok].astype(np.uint32)))
    c.append(("every binary16", HALF2FLOAT, np.arange(65536, dtype=np.uint32), None))
    c.append(("0..255", UNORM8, np.arange(256, dtype=np.uint32), None))
    c.append(("every draw", NEG_LOG_1M, draws(), None))
    _cases = c
    return c


N_ARRAY_CASES = 22          # len(array_cases()), known without building them (test parametrisation)

_PI, _PIO2, _INF, _NAN = 0x40490FDB, 0x3FC90FDB, float("inf"), None
# (what, fn, a, b, expected bits; None: any NaN).  The project's specification where it differs from C's libm, or where C leaves the result open.
SPEC_PINS = [
    ("atan2_(+0, -0) = 0", ATAN2, 0.0, -0.0, 0), ("atan2_(-0, -0) = 0", ATAN2, -0.0, -0.0, 0), ("atan2_(-0, +0) = 0", ATAN2, -0.0, 0.0, 0),
    ("atan2_(-0, -1) = +pi", ATAN2, -0.0, -1.0, _PI), ("atan2_(+0, -1) = +pi", ATAN2, 0.0, -1.0, _PI),
    ("atan2_(inf, inf) is NaN", ATAN2, _INF, _INF, _NAN), ("atan2_(-inf, inf) is NaN", ATAN2, -_INF, _INF, _NAN),
    ("atan2_(inf, -inf) is NaN", ATAN2, _INF, -_INF, _NAN), ("atan2_(-inf, -inf) is NaN", ATAN2, -_INF, -_INF, _NAN),
    ("pow_(0, 0) = 0", POW, 0.0, 0.0, 0), ("pow_(-0, -1) = 0", POW, -0.0, -1.0, 0), ("pow_(-1, 2) = 0", POW, -1.0, 2.0, 0), ("pow_(-inf, 1) = 0", POW, -_INF, 1.0, 0),
    ("pow_(1, inf) is NaN", POW, 1.0, _INF, _NAN), ("pow_(1, -inf) is NaN", POW, 1.0, -_INF, _NAN), ("pow_(inf, 0) is NaN", POW, _INF, 0.0, _NAN),
    ("sin_(8192) is NaN", SIN, 8192.0, 0.0, _NAN), ("cos_(-8192) is NaN", COS, -8192.0, 0.0, _NAN), ("tan_(8192) is NaN", TAN, 8192.0, 0.0, _NAN),
    ("sincos_(8192).s is NaN", SINCOS_S, 8192.0, 0.0, _NAN), ("sincos_(-8192).c is NaN", SINCOS_C, -8192.0, 0.0, _NAN), ("sin_(inf) is NaN", SIN, _INF, 0.0, _NAN),
    ("cos_(8191.9995), the last argument below the domain end, is finite", COS, 8191.99951171875, 0.0, 0x3E95ACEC),
    ("asin_(2) = asin_(1) = pi/2", ASIN, 2.0, 0.0, _PIO2), ("asin_(-inf) = -pi/2", ASIN, -_INF, 0.0, _PIO2 | 0x80000000),
    ("acos_(2) = acos_(1) = 0", ACOS, 2.0, 0.0, 0), ("acos_(-2) = acos_(-1) = pi", ACOS, -2.0, 0.0, _PI), ("acos_(inf) = 0", ACOS, _INF, 0.0, 0),
    ("min_(NaN, 1) is NaN", MIN, float("nan"), 1.0, _NAN), ("min_(1, NaN) = 1", MIN, 1.0, float("nan"), 0x3F800000),
    ("max_(NaN, 1) is NaN", MAX, float("nan"), 1.0, _NAN), ("max_(1, NaN) = 1", MAX, 1.0, float("nan"), 0x3F800000),
    ("min_(+0, -0) = +0", MIN, 0.0, -0.0, 0), ("min_(-0, +0) = -0", MIN, -0.0, 0.0, 0x80000000),
    ("clamp_(NaN, 0, 1) is NaN", CLAMP_LO, float("nan"), 0.0, _NAN), ("clamp_(2, NaN, 1) = 1", CLAMP_LO, 2.0, float("nan"), 0x3F800000),
    ("exp_(-inf) = 0", EXP, -_INF, 0.0, 0), ("exp_(-103.2789) = 2^-149", EXP, -103.27892303466797, 0.0, 1), ("exp_(89) = inf", EXP, 89.0, 0.0, 0x7F800000),
    ("log_(-0) = -inf", LOG, -0.0, 0.0, 0xFF800000), ("log_(-1) is NaN", LOG, -1.0, 0.0, _NAN), ("log_(inf) = inf", LOG, _INF, 0.0, 0x7F800000),
    ("log_(2^-149) = -103.2789", LOG, 1e-45, 0.0, 0xC2CE8ED0),
    ("sanitize(NaN) = 0", SANITIZE, float("nan"), 0.0, 0), ("sanitize(-inf) = 0", SANITIZE, -_INF, 0.0, 0), ("sanitize(-0) = -0", SANITIZE, -0.0, 0.0, 0x80000000),
    ("floor2i(NaN) = INT_MIN", FLOOR2I, float("nan"), 0.0, 0x80000000), ("floor2i(2^31) = INT_MIN", FLOOR2I, 2147483648.0, 0.0, 0x80000000),
    ("floor2i(-0.5) = -1", FLOOR2I, -0.5, 0.0, 0xFFFFFFFF),
]


def pin_holds(got, want):
    return (got & 0x7FFFFFFF) > 0x7F800000 if want is None else got == want
