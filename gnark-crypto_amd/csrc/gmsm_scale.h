// Variable-base batch scalar multiplication: n points, each by a scalar of its own (the updates of an SRS ceremony).
//
// Replaces: mpcsetup.UpdateMonomialsG1 / UpdateMonomialsG2 (A[i] <- r^i A[i]), the slice cases of mpcsetup.UpdateValues
// (every point of a slice by one value) and the per-point ScalarMultiplication loops behind them (ecc/bn254/mpcsetup/
// mpcsetup.go:64-81, :366-381), which the reference runs one after another on one core; and the powers with zeros at the
// segment ends that linearCombinationsG1/G2 feed to their MultiExp (mpcsetup.go:396-447, :489-540). All six groups.
//
// Shape: one lane per point, one launch per chunk of SCALE_CHUNK points.
//   k_batch_scale   out[i] = s_i P_i (n Montgomery fr.Elements) or s P_i (one: every lane reads the same element, the
//                   digits agree across the wave and the walk does not diverge - lanes at infinity only sit idle)
//   k_scale_powers  out[i] = r^i P_i: r^i is made in the lane from the table of r^(2^b) (<= 40 products, as
//                   k_group_fft_twiddles); no n-element scalar vector exists. r^0 = 1, so out[0] = P_0 (also for r = 0)
//   k_zero_at       the zeros at ends[j] - 1 of the powers vector of the linear combinations (k_fft_pow_table makes it)
// Each lane: affine (Go layout) -> record, scalar out of Montgomery form, GLV split (glv_split), the joint walk of
// gmsm_walk.h over lazy XYZZ records with its three table entries in HBM, record out; k_batch_normalize
// (gmsm_fixedbase.h) then writes canonical affine limbs, infinity = (0, 0). GLV runs for every group, the Fp2 ones (G2 of
// BN254 and BLS12-381) included: their records go through the generic group law (add_g / double_g) and phi is two products.
// The table bounds the chunk: 3 records per lane, at most 3 * SCALE_CHUNK * 448 bytes (BLS12-381 G2) of scratch.
// Special cases: an input at infinity stays; scalar 0 has no digit and leaves the accumulator at infinity; r - 1 splits
// like any scalar and gives -P; either half may be negative (the table entry is negated, not the scalar).
// Precondition (as the reference's ScalarMultiplication = mulGLV): every input lies in the r-torsion.
#pragma once
#include "gmsm_fixedbase.h"
#include "gmsm_fft.h"
#include "gmsm_walk.h"

namespace gmsm {

static constexpr size_t SCALE_CHUNK = (size_t)1 << 18;  // lanes per launch: what the walk's table is sized for

// point `i` (Go-layout affine) multiplied by `s` (Montgomery) -> record i of `recs`; `lane` of `lanes` addresses the table
template <class U, class C, class FrP, bool GLV, bool INL, class GetScalar>
__device__ __forceinline__ void scale_lane(const void *__restrict__ points, size_t i, GetScalar scalar, void *__restrict__ recs,
                                           void *__restrict__ tab, size_t lane, size_t lanes) {
    using T = LzTraits<U>;
    const Affine<typename T::Sat> a = load_struct<Affine<typename T::Sat>>(points, i);
    UnsatElem<U> e;
    e.inf = a.is_infinity();
    if (!e.inf) {
        e.v.x = T::template from_sat<true>(a.x);
        e.v.y = T::template from_sat<true>(a.y);
        e.v.zz = e.v.zzz = lz_one((const U *)nullptr);
        walk_mul<U, C, FrP, GLV, INL>(e, walk_scalar<FrP, GLV>(scalar()), tab, lane, lanes);
    }
    lazy_store<U>(recs, i, e.v, e.inf);
}

// points [first, first + count): recs[i] = scalars[UNIFORM ? 0 : i] * points[i]
template <class U, class C, class FrP, bool GLV, bool INL, bool UNIFORM>
__global__ void __launch_bounds__(256) k_batch_scale(const void *__restrict__ points, size_t first, size_t count,
                                                     const Fp<FrP> *__restrict__ scalars, void *__restrict__ recs,
                                                     void *__restrict__ tab) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    const size_t i = first + t;
    scale_lane<U, C, FrP, GLV, INL>(points, i, [&]() { return fft_load(scalars, UNIFORM ? (size_t)0 : i); }, recs, tab, t, count);
}

// points [first, first + count): recs[i] = r^i * points[i], pw = powers r^(2^b)
template <class U, class C, class FrP, bool GLV, bool INL>
__global__ void __launch_bounds__(256) k_scale_powers(const void *__restrict__ points, size_t first, size_t count, FftPowers<FrP> pw,
                                                      void *__restrict__ recs, void *__restrict__ tab) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    const size_t i = first + t;
    scale_lane<U, C, FrP, GLV, INL>(points, i,
                                    [&]() {
                                        Fp<FrP> acc = Fp<FrP>::one();
#pragma nounroll
                                        for (int b = 0; b < 40; ++b)
                                            if ((i >> b) & 1) acc = fp_mul(acc, pw.p[b]);
                                        return acc;
                                    },
                                    recs, tab, t, count);
}

// a[ends[j] - 1] = 0, j < n_ends (ends[j] >= 1, checked by the caller)
template <class FrP>
__global__ void __launch_bounds__(256) k_zero_at(Fp<FrP> *__restrict__ a, const uint64_t *__restrict__ ends, size_t n_ends) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_ends) return;
    fft_store(a, (size_t)ends[j] - 1, Fp<FrP>::zero());
}

}  // namespace gmsm
