// Device self-check of the hand-expanded divisions (dispersion_core.h: recip_of / div_by, ray_core.h: recipf_of / divf_by) against the
// compiler's IEEE division, operand pair by operand pair, bit for bit.  Not on any product path: tests/test_gpu_boundary.py runs it, so that
// "the same instructions on the same operands" is a measured statement and the operand ranges the headers name are the ones checked.
#include "../../include/dsurftomo_amd.h"
#include "kernels.h"
#include "dispersion_core.h"
#include "ray_core.h"
#include "eikonal_core.h"

namespace dsa {

__device__ __forceinline__ unsigned long long sc_next(unsigned long long& s)
{
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    unsigned long long z = s;
    z ^= z >> 33; z *= 0xff51afd7ed558ccdull; z ^= z >> 33;
    return z;
}
// a double with a uniform mantissa, a random sign and an exponent drawn from [elo, ehi] (unbiased)
__device__ __forceinline__ double sc_f64(unsigned long long& s, int elo, int ehi)
{
    const unsigned long long r = sc_next(s), q = sc_next(s);
    const int e = elo + (int)(q % (unsigned long long)(ehi - elo + 1));
    const unsigned long long bits = ((r & 1ull) << 63) | ((unsigned long long)(e + 1023) << 52) | ((r >> 12) & 0xfffffffffffffull);
    return __longlong_as_double((long long)bits);
}
__device__ __forceinline__ float sc_f32(unsigned long long& s, int elo, int ehi)
{
    const unsigned long long r = sc_next(s), q = sc_next(s);
    const int e = elo + (int)(q % (unsigned long long)(ehi - elo + 1));
    const unsigned bits = ((unsigned)(r & 1ull) << 31) | ((unsigned)(e + 127) << 23) | ((unsigned)(r >> 41) & 0x7fffffu);
    return __uint_as_float(bits);
}

// out[0]: fp64 pairs tried, out[1]: fp64 quotients that differ; out[2], out[3]: the same for fp32.  Every denominator serves `share`
// numerators, as it does in the product (the layer product's norm, a ray's cell sizes); numerators also take the special values 0, -0,
// +inf and NaN now and then (v_div_fixup's business).
__global__ void k_selfcheck_divisions(unsigned long long seed, int per_thread, int share, int nlo64, int nhi64, int dlo64, int dhi64,
                                      int nlo32, int nhi32, int dlo32, int dhi32, unsigned long long* __restrict__ out)
{
    unsigned long long s = seed ^ ((unsigned long long)(blockIdx.x * blockDim.x + threadIdx.x) * 0x9e3779b97f4a7c15ull);
    unsigned long long n64 = 0, bad64 = 0, n32 = 0, bad32 = 0;
    for (int i = 0; i < per_thread; ++i) {
        const double d = sc_f64(s, dlo64, dhi64);
        const Recip R = recip_of(d);
        const float df = sc_f32(s, dlo32, dhi32);
        const RecipF Rf = recipf_of(df);
        for (int k = 0; k < share; ++k) {
            double x = sc_f64(s, nlo64, nhi64);
            float xf = sc_f32(s, nlo32, nhi32);
            const unsigned sp = (unsigned)(sc_next(s) & 255ull);
            if (sp == 0) { x = 0.0; xf = 0.0f; } else if (sp == 1) { x = -0.0; xf = -0.0f; }
            else if (sp == 2) { x = __longlong_as_double(0x7ff0000000000000ll); xf = __uint_as_float(0x7f800000u); }
            else if (sp == 3) { x = __longlong_as_double(0x7ff8000000000000ll); xf = __uint_as_float(0x7fc00000u); }
            const double a = x / d, b = div_by(x, R);
            const float af = xf / df, bf = divf_by(xf, Rf);
            ++n64; ++n32;
            const bool nan64 = a != a && b != b, nan32 = af != af && bf != bf;      // (NaN payloads are not part of the contract)
            if (!nan64 && __double_as_longlong(a) != __double_as_longlong(b)) ++bad64;
            if (!nan32 && __float_as_uint(af) != __float_as_uint(bf)) ++bad32;
        }
    }
    atomicAdd(out + 0, n64); atomicAdd(out + 1, bad64); atomicAdd(out + 2, n32); atomicAdd(out + 3, bad32);
}

// The node trip's arithmetic helpers (eikonal_core.h: sqrt_nonneg, min_canon, min3_sel) against their plain forms, bit for bit.
// out[0]: square roots tried, out[1]: that differ from sqrtf (outside the guard), out[2]: arguments the guard sent to the plain sqrtf;
// out[3]: minima tried, out[4]: that differ.  Half of the square roots take the two-sided step's discriminant as solve_regular forms it -- all four
// variants of (a, b, c), cell sizes of 1e-5 .. 1e-1 rad, radii 6371 +- 100 km, slowness 0.1 .. 1 s/km, time differences of 0 and 1e-12 .. 1e3 s, with
// exact zeros and cancellation (the difference set to the value that makes c vanish) --, half a positive number of any exponent, with 0, +inf,
// NaN and the range below 2^-96 now and then.  The minima take travel times (1e-12 .. 1e3 s), +inf, equal operands and a quiet NaN.
__global__ void k_selfcheck_trip(unsigned long long seed, int per_thread, unsigned long long* __restrict__ out)
{
    unsigned long long s = seed ^ ((unsigned long long)(blockIdx.x * blockDim.x + threadIdx.x) * 0x9e3779b97f4a7c15ull);
    unsigned long long nsq = 0, badsq = 0, guarded = 0, nmin = 0, badmin = 0;
    const float nanq = __uint_as_float(0x7fc00000u);
    for (int i = 0; i < per_thread; ++i) {
        float x;
        const unsigned long long pick = sc_next(s);
        if (pick & 1ull) {
            const float ri = 6271.0f + 200.0f * (float)((pick >> 8) & 0xffffull) * (1.0f / 65535.0f);
            const float risti = ri * (0.1f + 0.9f * (float)((pick >> 24) & 0xffffull) * (1.0f / 65535.0f));
            const float dnx = fabsf(sc_f32(s, -17, -4)), dnz = fabsf(sc_f32(s, -17, -4));        // 7.6e-6 .. 0.125 rad
            const float slown = 0.1f + 0.9f * (float)((pick >> 40) & 0xffffull) * (1.0f / 65535.0f);
            const int var = (int)((pick >> 1) & 3ull);
            const bool sx = (var & 1) != 0, sz = (var & 2) != 0, both = sx && sz, one = sx != sz;
            const float s2 = sq(slown), A = sq(ri * dnx), B = sq(risti * dnz), s2A = A * s2, s2B = B * s2;
            const float U = (sx && !sz) ? B : A;
            const float S = (sx && !sz) ? 4.0f * s2A : (sz ? 4.0f * s2B : s2B);
            const float a00 = A + B;
            const float a = sx ? (sz ? 4.0f * a00 : 4.0f * A + 9.0f * B) : (sz ? 4.0f * B + 9.0f * A : a00);
            float em = sc_f32(s, -40, 10);                                                         // 9e-13 .. 2e3 s, either sign
            const unsigned sp = (unsigned)((pick >> 3) & 31ull);
            if (sp == 0) em = 0.0f;
            else if (sp < 8) em = (sp & 1u ? 1.0f : -1.0f) * sqrt_pos(S) * (1.0f + (float)((int)(sp >> 1) - 2) * 1.1920929e-7f);      // c = U (em^2 - S) cancels
            else if (sp < 16) {                                                                   // the discriminant itself cancels: b^2 = 4 a c (a grazing front)
                const float f = both ? 8.0f : (one ? 6.0f : -2.0f), g4a = 4.0f * a * (both ? 4.0f : 1.0f), den = g4a - sq(f) * U;
                if (den > 0.0f) em = (sp & 1u ? 1.0f : -1.0f) * sqrtf(g4a * S / den) * (1.0f + (float)((int)(sp >> 1) - 6) * 1.1920929e-7f);
            }
            const float b = (both ? 8.0f : (one ? 1.0f : -2.0f)) * (((one ? 6.0f : 1.0f) * em) * U);
            const float cc = (both ? 4.0f : 1.0f) * (U * (sq(em) - S));
            x = sq(b) - 4.0f * a * cc;
            if (x < 0.0f) x = 0.0f;
        } else {
            x = fabsf(sc_f32(s, -96, 100));
            const unsigned sp = (unsigned)((pick >> 3) & 1023ull);
            if (sp == 0) x = 0.0f; else if (sp == 1) x = kInf; else if (sp == 2) x = nanq;
            else if (sp < 6) x = fabsf(sc_f32(s, -126, -97));                                      // the guard's range
            else if (sp == 6) x = __uint_as_float((unsigned)(sc_next(s) & 0x7fffffull) | 1u);      // denormal
        }
        bool outside;
        const float h = sqrt_nonneg(x, &outside), plain = sqrtf(x);
        ++nsq;
        if (outside) ++guarded;
        else if (!(h != h && plain != plain) && __float_as_uint(h) != __float_as_uint(plain)) ++badsq;

        float t[3];
        const unsigned long long pm = sc_next(s);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            t[k] = fabsf(sc_f32(s, -40, 10));
            const unsigned sp = (unsigned)((pm >> (8 * k)) & 15ull);
            if (sp == 0) t[k] = kInf; else if (sp == 1 && k > 0) t[k] = t[0]; else if (sp == 2 && k > 0) t[k] = nanq;      // (the first operand is never NaN: see min3_sel)
        }
        const float m2 = min_canon(t[0], t[1]), p2 = fminf(t[0], t[1]);
        float p3 = t[0] < kInf ? t[0] : kInf;
        p3 = t[1] < p3 ? t[1] : p3;
        p3 = t[2] < p3 ? t[2] : p3;
        const float m3 = min3_sel(t[0], t[1], t[2]);
        nmin += 2;
        if (__float_as_uint(m2) != __float_as_uint(p2)) ++badmin;
        if (__float_as_uint(m3) != __float_as_uint(p3)) ++badmin;
    }
    atomicAdd(out + 0, nsq); atomicAdd(out + 1, badsq); atomicAdd(out + 2, guarded); atomicAdd(out + 3, nmin); atomicAdd(out + 4, badmin);
}

}  // namespace dsa

extern "C" int dsa_selfcheck_trip(unsigned long long seed, int millions, unsigned long long* out5)
{
    using namespace dsa;
    if (!out5 || millions < 1 || millions > 4096) return DSA_ERR_ARGUMENT;
    unsigned long long* d_out = nullptr;
    if (hipMalloc(&d_out, 5 * sizeof(unsigned long long)) != hipSuccess) return DSA_ERR_DEVICE;
    if (hipMemset(d_out, 0, 5 * sizeof(unsigned long long)) != hipSuccess) { (void)hipFree(d_out); return DSA_ERR_DEVICE; }
    const int per_thread = 64, threads = 256;
    const long long n = (long long)millions * 1000000ll;
    const int blocks = (int)((n + (long long)threads * per_thread - 1) / ((long long)threads * per_thread));
    hipLaunchKernelGGL(k_selfcheck_trip, dim3(blocks), dim3(threads), 0, 0, seed, per_thread, d_out);
    const hipError_t rc = hipMemcpy(out5, d_out, 5 * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    (void)hipFree(d_out);
    return rc == hipSuccess ? 0 : DSA_ERR_INTERNAL;
}

extern "C" int dsa_selfcheck_divisions(unsigned long long seed, int millions, const int* exponents8, unsigned long long* out4)
{
    using namespace dsa;
    if (!exponents8 || !out4 || millions < 1 || millions > 4096) return DSA_ERR_ARGUMENT;
    unsigned long long* d_out = nullptr;
    if (hipMalloc(&d_out, 4 * sizeof(unsigned long long)) != hipSuccess) return DSA_ERR_DEVICE;
    if (hipMemset(d_out, 0, 4 * sizeof(unsigned long long)) != hipSuccess) { (void)hipFree(d_out); return DSA_ERR_DEVICE; }
    const int share = 5, per_thread = 16, threads = 256;
    const long long pairs = (long long)millions * 1000000ll;
    const int blocks = (int)((pairs + (long long)threads * per_thread * share - 1) / ((long long)threads * per_thread * share));
    hipLaunchKernelGGL(k_selfcheck_divisions, dim3(blocks), dim3(threads), 0, 0, seed, per_thread, share, exponents8[0], exponents8[1], exponents8[2],
                       exponents8[3], exponents8[4], exponents8[5], exponents8[6], exponents8[7], d_out);
    const hipError_t rc = hipMemcpy(out4, d_out, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    (void)hipFree(d_out);
    return rc == hipSuccess ? 0 : DSA_ERR_INTERNAL;
}
