// electrical_ops.hpp -- the arithmetic of gr::electrical::PowerFactor and gr::electrical::SystemUnbalance (blocks/electrical/.../PowerEstimators.hpp:144-257), ONE
// definition for the host mirror blocks (gr4/blocks.hpp) and the device kernels (csrc/electrical.hip): the two domains of a block agree bit for bit on every
// input, the phase angle excepted (acos_of below, POWER_QUALITY.md).  T is float or double; every operation is IEEE + - * / abs compare in T, in the order
// written, nothing contracted, nothing reassociated.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define GR4_EL_HD __host__ __device__ __forceinline__
#else
#define GR4_EL_HD inline
#endif

namespace gr4::electrical_ops {

GR4_EL_HD float  abs_of(float x) { return __builtin_fabsf(x); }
GR4_EL_HD double abs_of(double x) { return __builtin_fabs(x); }

// ---- PowerFactor (:166-176)
// cos(phi) = P / S, 0 where S == 0 (either sign), then std::clamp(c, -1, 1) = (c < -1) ? -1 : (1 < c) ? 1 : c: a NaN stays NaN, -0.0 stays -0.0
template <typename T>
GR4_EL_HD T power_factor(T P, T S) {
    const T c = (S != T(0)) ? P / S : T(0);
    return (c < T(-1)) ? T(-1) : (T(1) < c) ? T(1) : c;
}
// phi = acos(cos(phi)).  The host calls std::acos in T like the reference; the device evaluates float samples in float64 on the float argument and rounds once,
// double samples with the device library's acos.  Each domain is compared with the oracle, never with the other.
GR4_EL_HD float acos_of(float c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (float)::acos((double)c);
#else
    return std::acos(c);
#endif
}
GR4_EL_HD double acos_of(double c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return ::acos(c);
#else
    return std::acos(c);
#endif
}

// ---- SystemUnbalance (:221-252), x(i) the value of phase i < n
// std::accumulate from T(0): ((0 + x_0) + x_1) + ...
template <typename T, typename Get>
GR4_EL_HD T sum_of(Get&& x, int n) {
    T s = T(0);
    for (int i = 0; i < n; ++i) s = s + x(i);
    return s;
}
template <typename T>
GR4_EL_HD T mean_of(T sum, int n) { return sum / static_cast<T>(n); }

// Voltage (:234-237): std::transform_reduce(first, last, T(0), std::max, |U_i - U_avg|).  The standard leaves the order of the reduction open; this is the left
// fold m = std::max(m, d_i) = (m < d_i) ? d_i : m from m = 0, which is how libstdc++ and libc++ evaluate it for fewer than four elements (the reference's two and
// three phases), kept for every phase count here.  A NaN deviation never replaces m.
template <typename T>
GR4_EL_HD void voltage_step(T& m, T x, T avg) {
    const T d = abs_of(x - avg);
    m         = (m < d) ? d : m;
}
// Current (:243-245): std::max_element with the comparator |a - I_avg| < |b - I_avg|, then |best - I_avg|: best starts at phase 0, so a NaN deviation of
// phase 0 stays (where every phase is +inf: NaN, the voltage form gives 0)
template <typename T>
GR4_EL_HD void current_step(T& best, T x, T avg) {
    if (abs_of(best - avg) < abs_of(x - avg)) best = x;
}
// (:239, :247) a division, then a multiplication; 0 unless avg > 0 (a NaN average: 0)
template <typename T>
GR4_EL_HD T percent_of(T dmax, T avg) { return (avg > T(0)) ? (dmax / avg) * T(100) : T(0); }

template <typename T, typename Get>
GR4_EL_HD T voltage_unbalance(Get&& x, int n) {
    const T avg = mean_of<T>(sum_of<T>(x, n), n);
    T       m   = T(0);
    for (int i = 0; i < n; ++i) voltage_step<T>(m, x(i), avg);
    return percent_of<T>(m, avg);
}
template <typename T, typename Get>
GR4_EL_HD T current_unbalance(Get&& x, int n) {
    const T avg  = mean_of<T>(sum_of<T>(x, n), n);
    T       best = x(0);
    for (int i = 1; i < n; ++i) current_step<T>(best, x(i), avg);
    return percent_of<T>(abs_of(best - avg), avg);
}

} // namespace gr4::electrical_ops
