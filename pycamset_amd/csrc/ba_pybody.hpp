// ba_pybody.hpp — Python's scalar semantics for user-block bodies translated from Python (pycamset_amd/block_translate.py).
//
// `//` and `%` floor (CPython's long division and float_divmod, bit for bit), `min(a, b)` / `max(a, b)` return the first argument
// unless the second one wins a plain comparison (so a NaN in first place survives, one in second place does not).  Included by a
// generated translation unit that holds translated bodies; also compiles as plain host C++ (the translator's differential tests).
#pragma once
#if defined(__HIPCC__) || defined(__HIPCC_RTC__)
#define PCS_PY_HD __host__ __device__
#else
#include <cmath>
#define PCS_PY_HD
#endif

namespace pcs_py {

PCS_PY_HD inline int floordiv(const int a, const int b) {
    const int q = a / b;
    return (q * b != a && ((a < 0) != (b < 0))) ? q - 1 : q;
}
PCS_PY_HD inline int mod(const int a, const int b) {
    const int r = a % b;
    return (r != 0 && ((r < 0) != (b < 0))) ? r + b : r;
}
PCS_PY_HD inline double mod(const double a, const double b) {
    double m = fmod(a, b);
    if (m != 0.0) {
        if ((b < 0.0) != (m < 0.0)) m += b;
    } else {
        m = copysign(0.0, b);
    }
    return m;
}
PCS_PY_HD inline double floordiv(const double a, const double b) {
    const double m = fmod(a, b);
    double d = (a - m) / b;
    if (m != 0.0 && ((b < 0.0) != (m < 0.0))) d -= 1.0;
    if (d != 0.0) {
        const double f = floor(d);
        return (d - f > 0.5) ? f + 1.0 : f;
    }
    return copysign(0.0, a / b);
}
PCS_PY_HD inline double min2(const double a, const double b) { return b < a ? b : a; }
PCS_PY_HD inline double max2(const double a, const double b) { return b > a ? b : a; }
PCS_PY_HD inline int min2(const int a, const int b) { return b < a ? b : a; }
PCS_PY_HD inline int max2(const int a, const int b) { return b > a ? b : a; }

}  // namespace pcs_py
