"""Known answers of tests/converter_oracle.py: the values a C++ compiler gives for the reference's expressions (ConverterBlocks.hpp), and the definitions
CONVERTERS.md adds where the reference is undefined."""
import numpy as np
import pytest

import converter_oracle as CO


def _sc(value, t, scale, r):
    return CO.scaling_convert(np.array([value], t), scale, r)[0]


def test_scaling_convert_multiplies_in_the_promoted_type():
    assert _sc(200, np.uint8, 200, np.float32) == np.float32(40000.0)  # narrowing the product to uint8 first would give 64
    assert _sc(-300, np.int16, 300, np.int32) == -90000
    assert _sc(-300, np.int16, 300, np.int16) == -24464  # integer -> integer narrows modulo 2^16
    assert _sc(200, np.uint8, 200, np.uint8) == 40000 % 256
    assert _sc(3, np.int8, -5, np.uint16) == 65536 - 15


def test_integer_to_float_rounds_once():
    v = 2 ** 60 + 2 ** 36 + 1
    got = _sc(v, np.int64, 1, np.float32)
    assert got == np.float32(float.fromhex("0x1.000002p+60"))
    assert np.float32(np.float64(v)) == np.float32(float.fromhex("0x1p+60"))  # the detour through double rounds twice
    assert CO.convert(np.array([v], np.int64), np.float32)[0] == got
    assert CO.convert(np.array([2 ** 24 + 1], np.int32), np.float32)[0] == np.float32(2 ** 24)  # ties to even


def test_float_to_integer_truncates_saturates_and_maps_nan_to_zero():
    x = np.array([1.9, -1.9, 127.9, 128.0, -128.9, -129.0, 1e10, -1e10, np.inf, -np.inf, np.nan, -0.0], np.float32)
    assert CO.convert(x, np.int8).tolist() == [1, -1, 127, 127, -128, -128, 127, -128, 127, -128, 0, 0]
    assert CO.convert(x, np.uint8).tolist() == [1, 0, 127, 128, 0, 0, 255, 0, 255, 0, 0, 0]
    assert CO.convert(np.array([2147483648.0, -2147483648.0, 2147483520.0], np.float32), np.int32).tolist() == [2 ** 31 - 1, -2 ** 31, 2147483520]
    assert CO.convert(np.array([9223372036854775808.0, 1e19, 18446744073709551616.0], np.float64), np.uint64).tolist() == [2 ** 63, 10 ** 19, 2 ** 64 - 1]
    assert CO.cast_scalar(1e6, np.int16) == 32767 and CO.cast_scalar(-2.7, np.int16) == -2 and CO.cast_scalar(float("nan"), np.uint8) == 0


def test_signed_overflow_wraps():
    assert _sc(65535, np.uint16, 65535, np.int64) == 65535 * 65535 - 2 ** 32  # uint16 * uint16 is an int product past 2^31
    assert _sc(2 ** 31 - 1, np.int32, 2, np.int64) == -2
    assert _sc(2 ** 62, np.int64, 4, np.int64) == 0
    assert CO.abs_(np.array([-2 ** 31], np.int32))[0] == -2 ** 31
    assert CO.abs_(np.array([-2 ** 63], np.int64))[0] == -2 ** 63


def test_abs():
    assert CO.abs_(np.array([200, 128, 127, 255], np.uint8)).tolist() == [56, 128, 127, 1]  # through int8, narrowed back to uint8
    assert CO.abs_(np.array([-128, -127, 5], np.int8)).tolist() == [-128, 127, 5]
    assert CO.abs_(np.array([0x80000000, 0xFFFFFFFF], np.uint32)).tolist() == [0x80000000, 1]
    f = CO.abs_(np.array([-0.0, -np.inf, -1.5], np.float32))
    assert f.view(np.uint32).tolist() == np.array([0.0, np.inf, 1.5], np.float32).view(np.uint32).tolist()
    assert not np.signbit(CO.abs_(np.array([-np.nan], np.float64)))[0]
    z = np.array([3 + 4j, complex(np.inf, np.nan), complex(np.nan, -np.inf), complex(np.nan, 1), 3e38 + 3e38j], np.complex64)
    got = CO.abs_(z)
    assert got.dtype == np.float32 and got[0] == 5 and got[1] == np.inf and got[2] == np.inf and np.isnan(got[3]) and got[4] == np.inf
    assert CO.abs_(np.array([1e308 + 1e308j], np.complex128))[0] == np.hypot(1e308, 1e308) < np.inf


def test_angle_conversions_are_a_division_then_a_multiplication():
    x = np.linspace(0.1, 6.3, 100000, dtype=np.float32)
    want = (x / np.float32(np.pi)) * np.float32(180)
    assert np.array_equal(CO.radians_to_degree(x), want) and want.dtype == np.float32
    a = np.mean(x * np.float32(180 / np.pi) != want)
    b = np.mean(x * (np.float32(1) / np.float32(np.pi)) * np.float32(180) != want)
    assert 0.25 < a < 0.5 and 0.05 < b < 0.25, (a, b)  # the shortcuts differ on about 36 % and 13 % of these values
    d = np.linspace(-720, 720, 1001, dtype=np.float64)
    assert np.array_equal(CO.degree_to_radians(d), (d / 180.0) * np.pi)


def test_arg_keeps_signed_zeros():
    z = np.array([complex(-0.0, -0.0), complex(-0.0, 0.0), complex(0.0, -0.0), complex(0.0, 0.0), -1 + 0j, 1j], np.complex64)
    got = CO.arg(z)
    pi = np.float32(np.pi)
    assert got.tolist() == [-pi, pi, 0.0, 0.0, pi, np.float32(np.pi / 2)]
    assert np.signbit(got[2]) and not np.signbit(got[3])


def test_compositions_and_interleaving():
    z = CO.mag_phase_to_complex(np.array([2.0, 1.0], np.float32), np.array([0.0, np.pi / 2], np.float32))
    assert z.dtype == np.complex64 and z[0] == 2 and z[1].imag == 1 and abs(z[1].real) < 1e-7
    c = np.array([1.5 - 2.5j, 300 - 40000j, complex(np.nan, np.inf)], np.complex64)
    assert CO.complex_to_interleaved(c, np.int8).tolist() == [1, -2, 127, -128, 0, 127]
    assert CO.complex_to_interleaved(c, np.int16).tolist() == [1, -2, 300, -32768, 0, 32767]
    i = np.array([-32768, 32767, 3, -4], np.int16)
    assert CO.interleaved_to_complex(i, np.complex64).tolist() == [complex(-32768, 32767), complex(3, -4)]
    assert CO.run("ToRealImag", (c,))[1].tolist()[:2] == [-2.5, -40000.0]
    assert CO.run("RealImagToComplex", (np.array([1.0]), np.array([-2.0])))[0].tolist() == [1 - 2j]


@pytest.mark.parametrize("kind,count", [("Convert", 100), ("ScalingConvert", 100), ("Abs", 12), ("Real", 2), ("Imag", 2), ("Arg", 2), ("RadiansToDegree", 2), ("DegreeToRadians", 2),
                                        ("ToRealImag", 2), ("RealImagToComplex", 2), ("ToMagPhase", 2), ("MagPhaseToComplex", 2), ("ComplexToInterleaved", 8),
                                        ("InterleavedToComplex", 8)])
def test_accepted_pairs(kind, count):
    assert len(CO.accepted_pairs(kind)) == count


def test_ulp_distance():
    a = np.array([1.0, 0.0, -0.0, np.nan, np.inf, 1.0], np.float32)
    b = np.array([np.nextafter(np.float32(1), np.float32(2)), -0.0, np.float32(1e-45), np.nan, np.finfo(np.float32).max, np.nan], np.float32)
    assert CO.ulp_distance(a, b).tolist() == [1, 0, 1, 0, 1, np.inf]
    c = np.array([1.0, -np.pi, 0.0, -1.0, np.inf], np.float64)  # float64: exact down to one unit (the ordered integers do not fit a float64)
    d = np.array([np.nextafter(1.0, 2.0), np.nextafter(np.nextafter(-np.pi, 0.0), 0.0), -5e-324, 1.0, -np.inf], np.float64)
    assert CO.ulp_distance(c, d).tolist() == [1, 2, 1, 2.0 * 0x3FF0000000000000, 2.0 * 0x7FF0000000000000]
