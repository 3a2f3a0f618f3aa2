// Host build of drone_rl_amd/csrc/trig.h for tests/test_trig_host.py.
#include <cstdint>

#include "../../drone_rl_amd/csrc/trig.h"

extern "C" void trig_sincos(int64_t n, const double *x, double *s, double *c) {
    for (int64_t i = 0; i < n; ++i) {
        const dr::SinCos t = dr::sincos_medium(x[i]);
        s[i] = t.s;
        c[i] = t.c;
    }
}

extern "C" void trig_sincosf(int64_t n, const float *x, float *s, float *c) {
    for (int64_t i = 0; i < n; ++i) {
        const dr::SinCosF t = dr::sincosf_medium(x[i]);
        s[i] = t.s;
        c[i] = t.c;
    }
}

// The range predicates that choose between the fast path and the library.
extern "C" void trig_fast_range(int64_t n, const double *x, uint8_t *out) {
    for (int64_t i = 0; i < n; ++i) out[i] = dr::sincos_fast_range(x[i]);
}

extern "C" void trig_fast_rangef(int64_t n, const float *x, uint8_t *out) {
    for (int64_t i = 0; i < n; ++i) out[i] = dr::sincosf_fast_range(x[i]);
}
