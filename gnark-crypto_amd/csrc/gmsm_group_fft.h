// The inverse FFT over G1 points that turns an SRS into its Lagrange form (ToLagrangeG1).
//
// Replaces: kzg.ToLagrangeG1 with computeTwiddlesInv, difFFTG1, bitReverse and the 1/n scaling (ecc/bn254/kzg/utils.go:25-
// 64, :66-95, :97-108, :117-180), for the G1 groups of BN254, BLS12-381 and BW6-761. out[i] = (1/n) sum_j w^(-ij) P_j with
// w = fr.Generator(n), in natural order. Every output is a group element and k_batch_normalize writes its unique canonical
// affine form, so any evaluation order gives the reference's limbs.
//
// Shape: one launch per radix-2 DIF stage over lazy XYZZ records in HBM. A stage of 2^20 BN254 records moves ~300 MB (tens
// of us) and multiplies 2^19 points by twiddles (~2600 field products each): the kernels are bound by the products, so
// the work goes into the scalar multiplication, not into fusing stages in LDS.
//   k_group_fft_twiddles  the n/2 twiddles w^-j, the n/2 first-stage twiddles w^-i / n and 1/n, GLV-split once per call
//   k_group_fft_load      affine (Go layout, or the packed lazy form of registered bases) -> records
//   k_group_fft_stage     stage s: a' = a + b, b' = (a - b) w^-(i 2^s) (complete XYZZ addition), then the twiddle product;
//                         stage 0 out of place, the others in place, the last one into bit-reversed positions (bitReverse)
//   k_batch_normalize     (gmsm_fixedbase.h) records -> canonical affine, infinity = (0, 0)
//
// Stage classes (stage s has 2^s blocks of 2m = n / 2^s points; butterfly (k, i): k the block, i < m, twiddle index i 2^s):
//   wave-uniform  2^s >= 64: lane t takes block k = t mod 2^s at i = t / 2^s, so the 64 lanes of a wave share i and
//                 the twiddle - the same table entry (a broadcast load), the same digits, no divergence in the walk;
//                 a wave at i = 0 (twiddle 1) skips the product as a whole
//   per-lane      2^s < 64 (the first six stages): lane t takes i = t mod m of block t / m; the digits differ per lane.
//                 The walk is the same code; an addition runs for the wave when any lane has a non-zero digit, so the
//                 cost is dbl + add per step instead of dbl + 3/4 add
// Scalar multiplication (GLV, GMSM_LAGRANGE_GLV=1): the twiddle s = k1 + k2 lambda, |k1|, |k2| < 2^GLV_BITS, and
//   s P = k1 (+-P) + k2 (+-phi(P)), phi(X, Y, ZZ, ZZZ) = (beta X, Y, ZZ, ZZZ) - one product. A joint binary walk (Straus-
//   Shamir) from the top bit: one doubling, then one addition of T[b1 + 2 b2], T = {P1, P2, P1 + P2} (the reference's
//   mulGLV walks the same pair two bits at a time, ecc/bn254/g1.go:529-600). The three entries of a lane live in a
//   workspace table in HBM (one record-sized slot per lane and entry, read back by the lane that wrote it): a table in
//   registers does not fit BW6-761's 108-word records. GMSM_LAGRANGE_GLV=0: a plain binary walk over the full scalar.
//   The walk itself is walk_mul (gmsm_walk.h), shared with the variable-base batch of gmsm_scale.h.
// 1/n is folded into the first stage: b' takes w^-i / n, a' one extra product by 1/n - n/2 scalar multiplications
// instead of n. n = 1 has no stage: the input, normalised.
// Precondition (as the reference's ScalarMultiplication = mulGLV): every input lies in the r-torsion.
#pragma once
#include "gmsm_fixedbase.h"
#include "gmsm_fft.h"
#include "gmsm_walk.h"

#ifndef GMSM_LAGRANGE_GLV
#define GMSM_LAGRANGE_GLV 1
#endif

namespace gmsm {

// out[e], e < 2 half + 1: w^-e (e < half), w^-(e - half) / n (e < 2 half), 1/n (e = 2 half); pw = powers of w^-1
template <class FrP, bool GLV>
__global__ void __launch_bounds__(256) k_group_fft_twiddles(FftPowers<FrP> pw, Fp<FrP> ninv, size_t half,
                                                            WalkScalar<FrP, GLV> *__restrict__ out) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e > 2 * half) return;
    const size_t x = e < half ? e : e < 2 * half ? e - half : 0;
    Fp<FrP> acc = e < half ? Fp<FrP>::one() : ninv;
#pragma nounroll
    for (int b = 0; b < 40; ++b)
        if ((x >> b) & 1) acc = fp_mul(acc, pw.p[b]);
    out[e] = walk_scalar<FrP, GLV>(acc);
}

// points -> lazy XYZZ records (ZZ = ZZZ = 1; infinity: zero ZZ limbs)
template <class U, bool PACKED>
__global__ void __launch_bounds__(256) k_group_fft_load(const void *__restrict__ points, size_t n, void *__restrict__ recs) {
    using T = LzTraits<U>;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    XYZZL<U> r;
    bool inf;
    if constexpr (PACKED) {  // registered bases (k_convert_points): already in the lazy domain
        const UAffine<U> a = load_struct<UAffine<U>>(points, i);
        inf = uaffine_is_infinity(a);
        r.x = T::unpack(a.x);
        r.y = T::unpack(a.y);
    } else {
        const Affine<typename T::Sat> a = load_struct<Affine<typename T::Sat>>(points, i);
        inf = a.is_infinity();
        r.x = T::template from_sat<true>(a.x);
        r.y = T::template from_sat<true>(a.y);
    }
    r.zz = r.zzz = lz_one((const U *)nullptr);
    lazy_store<U>(recs, i, r, inf);
}

__device__ __forceinline__ size_t lag_bitrev(size_t i, unsigned log2n) {
    return log2n ? (size_t)(__brevll((unsigned long long)i) >> (64 - log2n)) : 0;
}

// DIF stage s of a transform of n = 2^log2n records, read from `src`, written to `dst`. One twiddle product per thread:
// n/2 threads (butterflies), n in stage 0, where 1/n is folded in - threads t < n/2 take b' = (a - b) w^-i / n
// (tw[half + i]), threads n/2 + t the same butterfly's a' = (a + b) / n (tw[2 half]: uniform). Two threads read every pair
// of stage 0, so it runs out of place (src != dst: a thread must not overwrite what the other has yet to read); the later
// stages, one thread per butterfly, run in place. They use tw[i 2^s] for b', skip the product for i = 0 and store a' as it
// is. The last stage (s = log2n - 1) writes to bit-reversed positions (bitReverse), out of place.
template <class P, class C, class FrP, bool GLV, bool INL>
__global__ void __launch_bounds__(256) k_group_fft_stage(const void *src, void *dst, unsigned log2n, unsigned s,
                                                         const WalkScalar<FrP, GLV> *__restrict__ tw, void *__restrict__ tab) {
    using U = FpU<P>;
    const size_t half = (size_t)1 << (log2n - 1);
    const bool first = s == 0;
    const size_t jobs = first ? 2 * half : half;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= jobs) return;
    const bool sum_job = t >= half;  // stage 0 only
    const size_t bt = sum_job ? t - half : t;
    const unsigned log2m = log2n - 1 - s;
    size_t k, i;
    if (s >= 6) {  // wave-uniform: 64 consecutive lanes = 64 blocks at the same i
        k = bt & (((size_t)1 << s) - 1);
        i = bt >> s;
    } else {       // per-lane
        k = bt >> log2m;
        i = bt & (((size_t)1 << log2m) - 1);
    }
    const size_t pa = (k << (log2m + 1)) | i, pb = pa + ((size_t)1 << log2m);
    UnsatElem<U> a = unsat_load<U>(src, pa), b = unsat_load<U>(src, pb);
    UnsatElem<U> d = a;
    add_u<P, INL>(a.v, a.inf, b.v, b.inf);  // a + b
    if (!b.inf) walk_negate_y(b.v);
    add_u<P, INL>(d.v, d.inf, b.v, b.inf);  // a - b
    const bool last = s + 1 == log2n;
    if (!first) lazy_store<U>(dst, last ? lag_bitrev(pa, log2n) : pa, a.v, a.inf);  // before the walk: frees a's registers
    UnsatElem<U> x = sum_job ? a : d;
    const size_t twi = sum_job ? 2 * half : first ? half + i : i << s;
    if (first || twi != 0) walk_mul<U, C, FrP, GLV, INL>(x, tw[twi], tab, t, jobs);  // else: twiddle 1
    const size_t px = sum_job ? pa : pb;
    lazy_store<U>(dst, last ? lag_bitrev(px, log2n) : px, x.v, x.inf);
}

}  // namespace gmsm
