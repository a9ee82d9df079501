"""numpy oracle of the fourteen type-converter blocks (blocks/basic/.../ConverterBlocks.hpp:13-277): what the reference's C++ computes for every in-range value,
bit for bit, and the definitions CONVERTERS.md gives where the reference is undefined (float -> integer saturates, NaN -> 0; signed overflow wraps).

The four transcendental kinds (Abs<complex>, Arg, ToMagPhase, MagPhaseToComplex) are evaluated in float64 and, for float samples, rounded once to float32."""
import numpy as np

KINDS = ["Convert", "ScalingConvert", "Abs", "Real", "Imag", "Arg", "RadiansToDegree", "DegreeToRadians", "ToRealImag", "RealImagToComplex", "ToMagPhase",
         "MagPhaseToComplex", "ComplexToInterleaved", "InterleavedToComplex"]
ARITH = [np.uint8, np.uint16, np.uint32, np.uint64, np.int8, np.int16, np.int32, np.int64, np.float32, np.float64]
INTERLEAVABLE = [np.float32, np.float64, np.int8, np.int16]
COMPLEX = [np.complex64, np.complex128]
FLOATS = [np.float32, np.float64]
TRANSCENDENTAL = ("Abs<complex>", "Arg", "ToMagPhase", "MagPhaseToComplex")


def base_of(dt):
    dt = np.dtype(dt)
    return np.dtype(np.float32) if dt == np.complex64 else np.dtype(np.float64) if dt == np.complex128 else dt


def complex_of(dt):
    return np.dtype(np.complex64) if np.dtype(dt) == np.float32 else np.dtype(np.complex128)


def accepted_pairs(kind):
    """(in_dtype, out_dtype) pairs the templates' requires clauses admit"""
    if kind in ("Convert", "ScalingConvert"):
        return [(np.dtype(t), np.dtype(r)) for t in ARITH for r in ARITH]
    if kind == "Abs":
        return [(np.dtype(t), base_of(t)) for t in ARITH + COMPLEX]
    if kind in ("Real", "Imag", "Arg", "ToRealImag", "ToMagPhase"):
        return [(np.dtype(t), base_of(t)) for t in COMPLEX]
    if kind in ("RadiansToDegree", "DegreeToRadians"):
        return [(np.dtype(t), np.dtype(t)) for t in FLOATS]
    if kind in ("RealImagToComplex", "MagPhaseToComplex"):
        return [(np.dtype(t), complex_of(t)) for t in FLOATS]
    if kind == "ComplexToInterleaved":
        return [(np.dtype(t), np.dtype(r)) for t in COMPLEX for r in INTERLEAVABLE]
    if kind == "InterleavedToComplex":
        return [(np.dtype(t), np.dtype(r)) for t in INTERLEAVABLE for r in COMPLEX]
    raise ValueError(kind)


def promoted(dt):
    """the type of T() * T() in C++: int for everything narrower"""
    dt = np.dtype(dt)
    return np.dtype(np.int32) if dt.kind in "iu" and dt.itemsize < 4 else dt


def cast(v, out_dtype):
    """static_cast<R>(v) on an array: integers narrow modulo 2^w, integer -> float rounds once, float -> float rounds to nearest, float -> integer truncates toward
    zero inside R's range and (DEVIATION: undefined in C++) saturates outside, NaN -> 0"""
    v = np.asarray(v)
    r = np.dtype(out_dtype)
    if v.dtype.kind == "f" and r.kind in "iu":
        info = np.iinfo(r)
        hi = v.dtype.type(2.0) ** (info.bits - (1 if r.kind == "i" else 0))  # 2^bits: exact
        lo = -hi if r.kind == "i" else v.dtype.type(0)
        inside = (v > lo) & (v < hi)  # False for NaN
        with np.errstate(invalid="ignore"):
            out = np.trunc(np.where(inside, v, 0)).astype(r)
        out[v >= hi] = info.max
        out[v <= lo] = info.min
        return out
    with np.errstate(over="ignore", invalid="ignore"):
        return v.astype(r)


def cast_scalar(value, dtype):
    """static_cast<T>(double value) with the same rules: how the scale setting becomes a T"""
    return cast(np.array([value], np.float64), dtype)[0]


def scaling_convert(x, scale, out_dtype):
    """static_cast<R>(input * scale), scale of type T, the product in the promoted type (DEVIATION: signed overflow wraps modulo 2^w)"""
    x = np.asarray(x)
    t, p = x.dtype, promoted(x.dtype)
    s = np.array([cast_scalar(scale, t)], t)
    if p.kind in "iu":
        u = np.dtype(f"u{p.itemsize}")
        prod = (x.astype(p).view(u) * s.astype(p).view(u)).view(p)
    else:
        with np.errstate(over="ignore", invalid="ignore"):
            prod = x * s
    return cast(prod, out_dtype)


def convert(x, out_dtype):
    return cast(np.asarray(x), out_dtype)


def abs_(x):
    x = np.asarray(x)
    if x.dtype.kind == "c":
        b = base_of(x.dtype)
        with np.errstate(over="ignore", invalid="ignore"):
            return np.hypot(x.real.astype(np.float64), x.imag.astype(np.float64)).astype(b)
    if x.dtype.kind == "f":
        return np.abs(x)
    s = x.view(np.dtype(f"i{x.dtype.itemsize}"))
    u = s.view(np.dtype(f"u{x.dtype.itemsize}"))
    return np.where(s < 0, np.negative(u), u).astype(u.dtype).view(x.dtype)  # abs of the minimum wraps to itself; the result is narrowed back to T


def arg(x):
    x = np.asarray(x)
    return np.arctan2(x.imag.astype(np.float64), x.real.astype(np.float64)).astype(base_of(x.dtype))


def radians_to_degree(x):
    x = np.asarray(x)
    t = x.dtype.type
    with np.errstate(over="ignore", invalid="ignore"):
        return (x / t(np.pi)) * t(180)


def degree_to_radians(x):
    x = np.asarray(x)
    t = x.dtype.type
    with np.errstate(over="ignore", invalid="ignore"):
        return (x / t(180)) * t(np.pi)


def mag_phase_to_complex(r, theta):
    r, theta = np.asarray(r), np.asarray(theta)
    out = np.empty(r.shape, complex_of(r.dtype))
    with np.errstate(over="ignore", invalid="ignore"):
        out.real = (r.astype(np.float64) * np.cos(theta.astype(np.float64))).astype(r.dtype)
        out.imag = (r.astype(np.float64) * np.sin(theta.astype(np.float64))).astype(r.dtype)
    return out


def complex_to_interleaved(x, out_dtype):
    x = np.asarray(x)
    out = np.empty(2 * x.size, out_dtype)
    out[0::2] = cast(x.real, out_dtype)
    out[1::2] = cast(x.imag, out_dtype)
    return out


def interleaved_to_complex(x, out_dtype):
    x = np.asarray(x)
    out = np.empty(x.size // 2, out_dtype)
    with np.errstate(over="ignore", invalid="ignore"):
        out.real = x[0::2].astype(base_of(out_dtype))
        out.imag = x[1::2].astype(base_of(out_dtype))
    return out


def run(kind, inputs, out_dtype=None, scale=1.0):
    """the outputs of one block as a tuple of arrays, one per output port"""
    a = inputs[0]
    if kind == "Convert":
        return (convert(a, out_dtype),)
    if kind == "ScalingConvert":
        return (scaling_convert(a, scale, out_dtype),)
    if kind == "Abs":
        return (abs_(a),)
    if kind == "Real":
        return (np.ascontiguousarray(a.real),)
    if kind == "Imag":
        return (np.ascontiguousarray(a.imag),)
    if kind == "Arg":
        return (arg(a),)
    if kind == "RadiansToDegree":
        return (radians_to_degree(a),)
    if kind == "DegreeToRadians":
        return (degree_to_radians(a),)
    if kind == "ToRealImag":
        return (np.ascontiguousarray(a.real), np.ascontiguousarray(a.imag))
    if kind == "RealImagToComplex":
        out = np.empty(a.shape, complex_of(a.dtype))
        out.real, out.imag = a, inputs[1]
        return (out,)
    if kind == "ToMagPhase":
        return (abs_(a), arg(a))
    if kind == "MagPhaseToComplex":
        return (mag_phase_to_complex(a, inputs[1]),)
    if kind == "ComplexToInterleaved":
        return (complex_to_interleaved(a, out_dtype),)
    if kind == "InterleavedToComplex":
        return (interleaved_to_complex(a, out_dtype),)
    raise ValueError(kind)


def is_transcendental(kind, in_dtype):
    return kind in ("Arg", "ToMagPhase", "MagPhaseToComplex") or (kind == "Abs" and np.dtype(in_dtype).kind == "c")


def ulp_distance(a, b):
    """distance in units in the last place between two float arrays of one dtype (0 where both are NaN, inf where one is; the ordered-integer distance, so it
    crosses zero and reaches the infinities), computed in integers: exact for float64 too"""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.dtype.kind == "f"
    it = np.dtype(f"i{a.dtype.itemsize}")

    def ordered(v):  # the integer whose order is the floats' order: negative floats mirrored (-0.0 -> 0)
        i = v.view(it).astype(np.int64)
        return np.where(i < 0, np.int64(np.iinfo(it).min) - i, i)
    oa, ob = ordered(a), ordered(b)
    hi, lo = np.maximum(oa, ob), np.minimum(oa, ob)
    d = (hi.view(np.uint64) - lo.view(np.uint64)).astype(np.float64)  # modulo 2^64: the true difference, which is below 2^64
    d = np.where(np.isnan(a) & np.isnan(b), 0.0, d)
    return np.where(np.isnan(a) ^ np.isnan(b), np.inf, d)


def special_values(dtype, rng, n_random=200):
    """the inputs of the parity tests: the type's extremes, +-0, NaN, +-inf, values outside every integer range and random ones"""
    dt = np.dtype(dtype)
    if dt.kind in "iu":
        info = np.iinfo(dt)
        sp = [info.min, info.max, 0, 1, info.max - 1, info.min + 1, info.max // 2, info.max // 2 + 1, 200 % (info.max + 1), 100]
        if dt.kind == "i":
            sp += [-1, -100, -300 if dt.itemsize > 1 else -3]
        big = [2 ** 24 + 1, 2 ** 31 + 5, 2 ** 53 + 1, 2 ** 60 + 2 ** 36 + 1, -(2 ** 60 + 2 ** 36 + 1)]
        sp += [b for b in big if info.min <= b <= info.max]
        rnd = rng.integers(info.min, info.max, n_random, dtype=dt, endpoint=True)
        small = rng.integers(max(info.min, -128), min(info.max, 127), n_random, dtype=dt, endpoint=True)
        return np.concatenate([np.array(sp, dtype=dt), rnd, small])
    if dt.kind == "f":
        fi = np.finfo(dt)
        sp = [0.0, -0.0, np.nan, np.inf, -np.inf, fi.max, -fi.max, fi.tiny, -fi.tiny, fi.tiny / 4, 1.0, -1.0, 0.5, -0.5, 0.999, -0.999, 1.5, 2.5, -1.5, -2.5,
              127.0, 127.5, 128.0, -128.0, -128.5, -129.0, 255.0, 255.9, 256.0, 32767.0, 32767.5, 32768.0, -32768.0, -32768.9, -32769.0, 65535.5, 65536.0,
              2147483520.0, 2147483648.0, -2147483648.0, -2147483904.0, 4294967040.0, 4294967296.0, 9223371487098961920.0, 9223372036854775808.0,
              -9223372036854775808.0, 18446742974197923840.0, 18446744073709551616.0, 1e10, -1e10, 1e19, -1e19, 1e20, 3e38, -3e38, 16777217.0]
        with np.errstate(over="ignore"):
            spa = np.array(sp, dtype=np.float64).astype(dt)
        rnd = (rng.standard_normal(n_random) * 10.0 ** rng.uniform(-3, 12, n_random)).astype(dt)
        small = (rng.standard_normal(n_random) * 100).astype(dt)
        return np.concatenate([spa, rnd, small])
    b = base_of(dt)
    re = special_values(b, rng, n_random)
    sp = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1.0, -1.0], b)
    grid_re, grid_im = np.meshgrid(sp, sp)
    out = np.empty(re.size + grid_re.size, dt)
    out.real[:re.size], out.imag[:re.size] = re, rng.permutation(re)
    out.real[re.size:], out.imag[re.size:] = grid_re.ravel(), grid_im.ravel()
    return out
