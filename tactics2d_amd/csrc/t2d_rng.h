// t2d_rng.h -- the counter random stream of the device generators (t2d_generate.hip: parking scenes, one stream per scene;
// t2d_trackgen.hip: racing tracks, one stream per attempt): splitmix64 over a 64-bit counter, the top 53 bits of each output as
// a uniform in [0, 1).  How a stream is keyed is the generator's business (include/t2d.h); draw k of a stream whose state is s
// is a function of s + (k + 1) * kStreamGamma alone, so any draw can be reached without the ones before it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "t2d_math.h"

namespace t2d {

constexpr uint64_t kStreamGamma = 0x9E3779B97F4A7C15ull;

// splitmix64's finaliser
T2D_DEV uint64_t stream_mix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

T2D_DEV double stream_unit(uint64_t z) { return (double)(z >> 11) * (1.0 / 9007199254740992.0); }

struct Stream {
    uint64_t s;
    T2D_DEV double u() {
        s += kStreamGamma;
        return stream_unit(stream_mix(s));
    }
    // draw k (0 = the next one) without advancing
    T2D_DEV double peek(uint64_t k) const { return stream_unit(stream_mix(s + (k + 1) * kStreamGamma)); }
    T2D_DEV double uniform(double a, double b) { return a + (b - a) * u(); }
    T2D_DEV double normal(double mean, double std) {  // Box-Muller, cosine branch
        const double u1 = 1.0 - u(), u2 = u();
        const double rad = __builtin_sqrt(-2.0 * log_det(u1));
        double sn, cs;
        sincos_det((2.0 * 3.141592653589793) * u2, sn, cs);
        return mean + std * (rad * cs);
    }
    T2D_DEV double trunc_gauss(double mean, double std, double lo, double hi) {  // :60-62
        return clipd(normal(mean, std), lo, hi);
    }
};

}  // namespace t2d
