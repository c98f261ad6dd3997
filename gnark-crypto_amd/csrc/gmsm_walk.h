// One lane's scalar multiplication e = [s] e over a lazy XYZZ record: the walk that the group FFT's twiddle products
// (gmsm_group_fft.h) and the variable-base batch (gmsm_scale.h) share, for both element types (FpU<P>, Fp2U<P>).
//
// Replaces (one point, one scalar): (*G1Jac).mulGLV / mulWindowed and their G2 twins (ecc/bn254/g1.go:529-600, g2.go).
// GLV: s = k1 + k2 lambda, |k1|, |k2| < 2^GLV_BITS, and s P = k1 (+-P) + k2 (+-phi(P)), phi(X, Y, ZZ, ZZZ) = (w X, Y, ZZ,
//   ZZZ) - one product (two for Fp2: w lies in Fp). A joint binary walk (Straus-Shamir) from the top bit: one doubling, then
//   one complete addition of T[b1 + 2 b2], T = {P1, P2, P1 + P2} (the reference walks the same pair two bits at a time). The
//   three entries of a lane live in a table in HBM (one record-sized slot per lane and entry, read back by the lane that
//   wrote it): a table in registers does not fit the 108-word records of BW6-761 or the 112-word ones of BLS12-381 G2.
// !GLV: a plain binary walk over the full scalar.
// The additions are the complete ones (lz_padd: P + P, P + (-P), infinity), so the accumulator meeting +-(a table entry) is
// handled where it happens. Lanes whose digits agree (one scalar for a whole wave) take the same branches: no divergence.
// Precondition (as the reference's ScalarMultiplication = mulGLV): the point lies in the r-torsion.
#pragma once
#include "gmsm_kernels.h"
#include "gmsm_glv.h"

namespace gmsm {

// One scalar as the walk reads it: the GLV halves (magnitudes, bit 0 / 1 of `neg` their signs) or the scalar itself, both
// in regular (not Montgomery) form.
template <class FrP, bool GLV>
struct WalkScalar {
    uint32_t k1[FrP::GLV_HL], k2[FrP::GLV_HL];
    uint32_t neg;
};
template <class FrP>
struct WalkScalar<FrP, false> {
    uint32_t s[FrP::N];
};

template <class FrP, bool GLV>
__device__ __forceinline__ WalkScalar<FrP, GLV> walk_scalar(const Fp<FrP> &mont) {
    const Fp<FrP> acc = fp_from_mont(mont);
    WalkScalar<FrP, GLV> t;
    if constexpr (GLV) {
        bool n1, n2;
        glv_split<FrP>(acc.l, t.k1, n1, t.k2, n2);
        t.neg = (n1 ? 1u : 0u) | (n2 ? 2u : 0u);
    } else {
#pragma unroll
        for (int k = 0; k < FrP::N; ++k) t.s[k] = acc.l[k];
    }
    return t;
}

// -P of a stored record. Prime field: 8q - y carry-passed, back into [0, 4q); Fp2: the reduced class's own subtraction
template <class P>
__device__ __forceinline__ void walk_negate_y(XYZZL<FpU<P>> &p) {
    p.y = fpu_negc<P, 8>(p.y);
    fpu_to_class_r(p.y);
}
template <class P>
__device__ __forceinline__ void walk_negate_y(XYZZL<Fp2U<P>> &p) {
    p.y = lz_sub(lz_zero((const Fp2U<P> *)nullptr), p.y);
}

template <int L>
__device__ __forceinline__ void walk_shl1(uint32_t (&k)[L]) {
#pragma unroll
    for (int i = L - 1; i > 0; --i) k[i] = (k[i] << 1) | (k[i - 1] >> 31);
    k[0] <<= 1;
}

// e = [sc] e. `tab` holds 3 record slots per lane (slot, slot + stride, slot + 2 stride), used by the GLV walk only.
template <class U, class C, class FrP, bool GLV, bool INL>
__device__ __forceinline__ void walk_mul(UnsatElem<U> &e, const WalkScalar<FrP, GLV> &sc, void *__restrict__ tab, size_t slot,
                                         size_t stride) {
    if (e.inf) return;
    XYZZL<U> acc;
    bool inf = true;
    if constexpr (GLV) {
        constexpr int HL = FrP::GLV_HL;
        XYZZL<U> p1 = e.v, p2 = e.v;
        p2.x = glv_mul_w<INL>(e.v.x, glv_w<U, C, INL>());  // phi
        if (sc.neg & 1u) walk_negate_y(p1);
        if (sc.neg & 2u) walk_negate_y(p2);
        lazy_store<U>(tab, slot, p1, false);
        lazy_store<U>(tab, slot + stride, p2, false);
        bool inf3 = false;
        lz_padd<INL>(p1, inf3, p2, false);
        lazy_store<U>(tab, slot + 2 * stride, p1, inf3);
        uint32_t k1[HL], k2[HL];
#pragma unroll
        for (int k = 0; k < HL; ++k) k1[k] = sc.k1[k], k2[k] = sc.k2[k];
        constexpr int SKIP = 32 * HL - FrP::GLV_BITS;  // bits above GLV_BITS are zero
#pragma unroll
        for (int b = 0; b < SKIP; ++b) walk_shl1(k1), walk_shl1(k2);
#pragma nounroll
        for (int b = 0; b < FrP::GLV_BITS; ++b) {
            if (!inf) acc = lz_pdbl<INL>(acc);
            const uint32_t sel = (k1[HL - 1] >> 31) | ((k2[HL - 1] >> 30) & 2u);
            walk_shl1(k1);
            walk_shl1(k2);
            if (sel) {
                const UnsatElem<U> t = unsat_load<U>(tab, slot + (sel - 1u) * stride);
                lz_padd<INL>(acc, inf, t.v, t.inf);
            }
        }
    } else {
        (void)tab, (void)slot, (void)stride;
        constexpr int N = FrP::N;
        uint32_t s[N];
#pragma unroll
        for (int k = 0; k < N; ++k) s[k] = sc.s[k];
        constexpr int SKIP = 32 * N - (int)FrP::BITS;
#pragma unroll
        for (int b = 0; b < SKIP; ++b) walk_shl1(s);
#pragma nounroll
        for (int b = 0; b < (int)FrP::BITS; ++b) {
            if (!inf) acc = lz_pdbl<INL>(acc);
            const bool bit = (s[N - 1] >> 31) != 0u;
            walk_shl1(s);
            if (bit) lz_padd<INL>(acc, inf, e.v, false);
        }
    }
    e.v = acc;
    e.inf = inf;
}

}  // namespace gmsm
