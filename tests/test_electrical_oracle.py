"""The numpy restatement of PowerFactor / SystemUnbalance (tests/electrical_oracle.py) pinned to the reference's own QA (blocks/electrical/test/
qa_PowerEstimators.cpp:183-292) and to the special-value consequences of its expressions (POWER_QUALITY.md)."""
import numpy as np
import pytest

import electrical_oracle as EO

V_RMS, I_RMS = 230.0, 10.0
OFFSETS = np.array([0.1, 0.2, 0.3], np.float32)  # phaseOffset of the QA, float


@pytest.mark.parametrize("dtype", EO.FLOATS)
def test_power_factor_of_the_reference_qa(dtype):
    """S = 2300, P = S cosf(x): the power factor within 1e-5 of cosf(x), the phase within 1e-5 of x (:196-226)"""
    cos_phi = np.cos(OFFSETS).astype(np.float32).astype(np.float64).astype(dtype)  # static_cast<T>(std::cos(float))
    S = np.full(3, V_RMS * I_RMS, dtype)
    P = (S * cos_phi).astype(dtype)
    pf, ph = EO.power_factor(P[:, None], S[:, None])
    assert pf.dtype == ph.dtype == np.dtype(dtype) and pf.shape == (3, 1)
    assert np.all(np.abs(pf[:, 0].astype(np.float64) - cos_phi.astype(np.float64)) < 1e-5)
    assert np.all(np.abs(ph[:, 0].astype(np.float64) - OFFSETS.astype(np.float64)) < 1e-5)


@pytest.mark.parametrize("dtype", EO.FLOATS)
def test_system_unbalance_of_the_reference_qa(dtype):
    """U = {230, 230 1.01f, 230 0.99f}, I = {10, 10 1.02f, 10 0.98f} (:236-291): the unbalances within 0.1 of their formula, the total power within 1 %"""
    f = np.float32
    U = np.array([V_RMS, f(V_RMS) * f(1.01), f(V_RMS) * f(0.99)], np.float64).astype(dtype)
    I = np.array([I_RMS, f(I_RMS) * f(1.02), f(I_RMS) * f(0.98)], np.float64).astype(dtype)
    P = (U.astype(np.float64) * I.astype(np.float64) * np.cos(OFFSETS).astype(np.float64)).astype(dtype)
    pt, uu, iu = EO.system_unbalance(U[:, None], I[:, None], P[:, None])

    def formula(x):
        x = x.astype(np.float64)
        avg = x.sum() / 3
        return np.abs(x - avg).max() / avg * 100
    assert abs(float(uu[0]) - formula(U)) < 0.1 and abs(float(uu[0]) - 1.0000013) < 1e-4
    assert abs(float(iu[0]) - formula(I)) < 0.1 and abs(float(iu[0]) - 1.9999981) < 1e-4
    want = float(P.astype(np.float64).sum())
    assert abs(float(pt[0]) - want) < 0.01 * want
    assert pt.dtype == uu.dtype == iu.dtype == np.dtype(dtype)


@pytest.mark.parametrize("dtype", EO.FLOATS)
def test_power_factor_consequences(dtype):
    """the table of POWER_QUALITY.md, sign bits included"""
    T = np.dtype(dtype).type
    inf, nan, pi = np.inf, np.nan, np.pi

    def one(P, S):
        pf, ph = EO.power_factor(np.array([P], dtype), np.array([S], dtype))
        return pf[0], ph[0]
    half_pi, full_pi = T(np.arccos(0.0)), T(pi)
    for S in (0.0, -0.0):
        for P in (1.0, -3.0, nan, inf, 0.0):
            pf, ph = one(P, S)
            assert pf == 0 and not np.signbit(pf) and ph == half_pi, (P, S)
    pf, ph = one(-0.0, 1.0)
    assert pf == 0 and np.signbit(pf) and ph == half_pi
    assert one(3.0, 2.0) == (T(1), T(0))
    pf, ph = one(-5.0, 2.0)
    assert pf == -1 and ph == full_pi
    pf, ph = one(1.0, inf)
    assert pf == 0 and not np.signbit(pf) and ph == half_pi
    for P, S in ((inf, inf), (-inf, inf), (nan, 1.0), (1.0, nan), (nan, nan), (nan, inf)):
        pf, ph = one(P, S)
        assert np.isnan(pf) and np.isnan(ph), (P, S)
    pf, ph = one(inf, 1.0)
    assert pf == 1 and ph == 0
    sub = np.finfo(dtype).smallest_subnormal
    pf, ph = one(sub, 1.0)
    assert pf == sub and ph == half_pi


@pytest.mark.parametrize("dtype", EO.FLOATS)
@pytest.mark.parametrize("n_phases", [2, 3])
def test_unbalance_consequences(dtype, n_phases):
    inf, nan = np.inf, np.nan
    fi = np.finfo(dtype)

    def both(*x):
        a = np.array(x, dtype)[:, None]
        return EO.voltage_unbalance(a)[0], EO.current_unbalance(a)[0]
    rest = [230.0] * (n_phases - 2)
    for k in range(n_phases):  # a NaN in any phase: avg = NaN, the output is 0
        x = [230.0] * n_phases
        x[k] = nan
        assert both(*x) == (0, 0)
    u, i = both(inf, 230.0, *rest)  # avg = +inf with a finite phase: NaN
    assert np.isnan(u) and np.isnan(i)
    u, i = both(*([inf] * n_phases))  # every phase +inf: the one input on which the two forms differ
    assert u == 0 and np.isnan(i)
    assert both(-230.0, -231.0, *[-1.0] * (n_phases - 2)) == (0, 0)  # avg <= 0
    assert both(0.0, -0.0, *[0.0] * (n_phases - 2)) == (0, 0)
    assert both(-inf, 230.0, *rest) == (0, 0)  # avg = -inf
    assert both(inf, -inf, *rest) == (0, 0)    # avg = NaN
    u, i = both(fi.max, fi.max, *[fi.max] * (n_phases - 2))  # the sum overflows: avg = +inf, every phase finite
    assert np.isnan(u) and np.isnan(i)
    u, i = both(230.0, 232.3, *rest)
    assert u == i and 0 < u < 1.1
    pt = EO.total_power(np.array([[-0.0]] * n_phases, dtype))
    assert pt[0] == 0 and not np.signbit(pt[0])  # ((0 + -0) + -0): +0


@pytest.mark.parametrize("dtype", EO.FLOATS)
@pytest.mark.parametrize("n_phases", [2, 3])
def test_the_two_unbalance_forms_differ_only_where_every_phase_is_inf(dtype, n_phases):
    """transform_reduce / max against max_element / comparator on the Cartesian grid of the 14 special values"""
    g = EO.grid(dtype, n_phases)
    assert g.shape == (n_phases, 14 ** n_phases)
    u, i = EO.voltage_unbalance(g), EO.current_unbalance(g)
    u8 = np.dtype(f"u{np.dtype(dtype).itemsize}")
    differ = ~((u.view(u8) == i.view(u8)) | (np.isnan(u) & np.isnan(i)))
    all_inf = np.all(np.isposinf(g), axis=0)
    assert np.array_equal(differ, all_inf) and all_inf.sum() == 1
    k = int(np.nonzero(all_inf)[0][0])
    assert u[k] == 0 and np.isnan(i[k])


def test_phase_inputs_cover_the_domain():
    for dtype in EO.FLOATS:
        P, S = EO.phase_inputs(dtype)
        pf, ph = EO.power_factor(P, S)
        fin = pf[~np.isnan(pf)]
        assert fin.min() == -1 and fin.max() == 1 and np.any(np.signbit(pf) & (pf == 0)) and np.isnan(pf).any()
        one = np.dtype(dtype).type(1)
        assert np.any(pf == np.nextafter(one, one - one)) and np.any(pf == -np.nextafter(one, one - one))
        assert np.all((ph[~np.isnan(ph)] >= 0) & (ph[~np.isnan(ph)] <= np.dtype(dtype).type(np.pi)))
        assert EO.ulp_distance(ph, ph).max() == 0 and EO.same_bits(pf, pf.copy())
