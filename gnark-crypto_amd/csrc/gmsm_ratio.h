// PLONK's accumulating-ratio polynomials and fr.BatchInvert on the device: the step between the FFTs and the commitments of
// a prover whose wire polynomials stay in HBM.
//
// Replaces, with identical results (every output is a uniquely determined element of Fr, stored canonically in Montgomery
// form, so neither the order of evaluation nor the way a vector is cut shows):
//   BuildRatioCopyConstraint             ecc/bn254/fr/iop/ratios.go:136-246
//   BuildRatioShuffledVectors            ratios.go:45-127
//   getSupportIdentityPermutation        ratios.go:320-361  (never materialised, see below)
//   putInExpectedFormFromLagrangeRegular ratios.go:248-273  (the FFT and bit-reverse kernels of gmsm_fft.h, same stream)
//   fr.BatchInvert                       ecc/bn254/fr/element.go:658-687 (out_i = 1/a_i, and 0 where a_i = 0)
// and the twins of BLS12-381 and BW6-761 (same templates, other scalar fields).
//
// Departures from the reference, all of them here:
//   * The inputs of the two ratio builders are in LAGRANGE basis (either layout, a flag per polynomial). The reference's
//     ToLagrange on the inputs (polynomial.go:287-318) stays with the wrappers, through the FFT entries.
//   * The support S[p] = g^(p div n) w^(p mod n) (m n elements in the reference) is not built: w^k is read from the domain's
//     resident twiddles (which hold k < n/2; w^(k + n/2) = -w^k) and g^j from a table of m entries that carries beta.
//   * A permutation value outside [0, m n) is refused (GMSM_ERR_ARG naming the first such index); the reference panics
//     with an index out of range.
//   * The reference inverts the denominators in chunks (ratios.go:230-238); BatchInvert returns 0 for 0 whatever the
//     chunk, so the chunking does not show and none is reproduced: Z_i = N_i inv0(D_i), and once some d_k = 0 every later
//     D_i is 0 and Z_i = 0, as in the reference.
//
// Shape on the GPU, with no flag, spin or grid barrier between workgroups:
//   1. k_ratio_factors_*  one lane per index i < n - 1: the numerator product b_i and the denominator product d_i over the m
//                         polynomials, written at i + 1 (position 0 holds one)
//   2. the inclusive prefix products N, D of both factor vectors in the launch shape of gmsm_poly.h, both vectors in the
//      same launches (two independent chains per lane: twice the ILP of a latency-bound field product):
//        k_ratio_lanes  each lane multiplies its T = 2^tb consecutive elements; the workgroup combines its 256 lanes with a
//                       log-step scan in LDS and writes every lane's in-tile prefix X_l and the tile's value S_t = X_255
//        k_ratio_lanes  the same kernel, fused, in one workgroup over the nt tile values: the carries C_t = S_0 .. S_t
//        k_ratio_apply  each lane's carry-in X_(l-1) C_(t-1), then the walk up its T elements, in place
//      A vector of one tile runs as one launch (k_ratio_lanes fused). T follows GMSM_OPT_POLY_LANE_BITS like the suffix scan.
//   3. k_ratio_invert   Montgomery's trick PER TILE: each lane multiplies its T elements (zeros skipped) and leaves the running
//                       products behind; the 256 lane products go up a product tree in LDS, ONE fp_inv per tile (lane 0; a
//                       Fermat ladder of ~1.5 log2 q products, which per lane would cost more than everything else
//                       together), back down the tree (inverse of a child = inverse of the parent times the sibling), and
//                       each lane walks back: out_i = inv * running_i [* N_i], inv *= a_i. Tiles are independent: no carry.
//                       Products per element: 1 up, 2 back, 1 for Z, and (3 * 255 + ~1.5 log2 q) / (256 T) for the tile.
#pragma once
#include <hip/hip_runtime.h>
#include "gmsm_context.h"
#include "gmsm_field.h"
#include "gmsm_fft.h"
#include "gmsm_poly.h"

namespace gmsm {

// iop.Basis / iop.Layout (ecc/bn254/fr/iop/polynomial.go:20-34)
constexpr int IOP_CANONICAL = 1, IOP_LAGRANGE = 2, IOP_LAGRANGE_COSET = 4;
constexpr uint32_t IOP_REGULAR = 8, IOP_BIT_REVERSE = 16;

// 2^s w^k for k < n from the domain's table tw[k] = 2^s w^k, k < half = n / 2 (lazy domain, gmsm_fft_lazy.h)
template <class FrP>
__device__ __forceinline__ Fp<FrP> ratio_omega(const Fp<FrP> *tw, size_t k, size_t half) {
    return k < half ? fft_load(tw, k) : fp_neg(fft_load(tw, k - half));
}

// Copy constraint (ratios.go:174-206). Lane p writes position p: one at 0, else for i = p - 1
//   b_i = prod_j (P_j[idx] + beta S[i + j n] + gamma),  d_i = prod_j (P_j[idx] + beta S[perm[i + j n]] + gamma)
// bg[j] = beta g^j 2^-s, so bg[j] ratio_omega(k) = beta S[j n + k]. *bad: the smallest index whose perm value is out of range.
template <class FrP>
__global__ void __launch_bounds__(256) k_ratio_factors_copy(const Fp<FrP> *__restrict__ entries, const uint32_t *__restrict__ layouts, size_t m,
                                                            size_t n, unsigned log2n, const long long *__restrict__ perm,
                                                            const Fp<FrP> *__restrict__ tw, const Fp<FrP> *__restrict__ bg, Fp<FrP> gamma,
                                                            Fp<FrP> *__restrict__ fnum, Fp<FrP> *__restrict__ fden,
                                                            unsigned long long *__restrict__ bad) {
    using Fr = Fp<FrP>;
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    Fr b = Fr::one(), d = Fr::one();
    if (p > 0) {
        const size_t i = p - 1, irev = fft_bitrev(i, log2n), half = n >> 1, mn = m * n;
        const Fr wi = ratio_omega(tw, i, half);
#pragma nounroll
        for (size_t j = 0; j < m; ++j) {
            const size_t idx = layouts[j] == IOP_BIT_REVERSE ? irev : i;
            const Fr pg = fp_add(fft_load(entries, j * n + idx), gamma);
            b = fp_mul(b, fp_add(pg, fp_mul(fft_load(bg, j), wi)));
            long long q = perm[i + j * n];
            if (q < 0 || (unsigned long long)q >= mn) {
                atomicMin(bad, (unsigned long long)(i + j * n));
                q = 0;
            }
            const size_t qj = (size_t)q >> log2n, qk = (size_t)q & (n - 1);
            d = fp_mul(d, fp_add(pg, fp_mul(fft_load(bg, qj), ratio_omega(tw, qk, half))));
        }
    }
    fft_store(fnum, p, b);
    fft_store(fden, p, d);
}

// Shuffled vectors (ratios.go:85-114): b_i = prod_j (beta - P_j[idx]), d_i = prod_j (beta - Q_j[idx]); layouts: m for the
// numerators, then m for the denominators.
template <class FrP>
__global__ void __launch_bounds__(256) k_ratio_factors_shuffled(const Fp<FrP> *__restrict__ num, const Fp<FrP> *__restrict__ den,
                                                                const uint32_t *__restrict__ layouts, size_t m, size_t n, unsigned log2n,
                                                                Fp<FrP> beta, Fp<FrP> *__restrict__ fnum, Fp<FrP> *__restrict__ fden) {
    using Fr = Fp<FrP>;
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    Fr b = Fr::one(), d = Fr::one();
    if (p > 0) {
        const size_t i = p - 1, irev = fft_bitrev(i, log2n);
#pragma nounroll
        for (size_t j = 0; j < m; ++j) {
            b = fp_mul(b, fp_sub(beta, fft_load(num, j * n + (layouts[j] == IOP_BIT_REVERSE ? irev : i))));
            d = fp_mul(d, fp_sub(beta, fft_load(den, j * n + (layouts[m + j] == IOP_BIT_REVERSE ? irev : i))));
        }
    }
    fft_store(fnum, p, b);
    fft_store(fden, p, d);
}

// The walk of lane g up its elements [g T, g T + T) of va and vb (m elements each) with carry-ins ya, yb (the prefix products
// just below the lane): v_i <- y = y v_i, in place.
template <class FrP>
__device__ __forceinline__ void ratio_lane_walk(Fp<FrP> *va, Fp<FrP> *vb, size_t m, size_t g, unsigned tb, Fp<FrP> ya, Fp<FrP> yb) {
    const size_t lo = g << tb, hi = min(lo + ((size_t)1 << tb), m);
#pragma nounroll
    for (size_t i = lo; i < hi; ++i) {
        ya = fp_mul(ya, fft_load(va, i));
        yb = fp_mul(yb, fft_load(vb, i));
        fft_store(va, i, ya);
        fft_store(vb, i, yb);
    }
}

// Passes 1 and 2 of the prefix products. One workgroup = one tile of TPB lanes x T elements of both vectors. FUSED = 0: writes
// X_l (xa, xb: one per lane) and S_t (sa, sb: one per tile). FUSED = 1 (one tile, gridDim.x == 1): the walk follows the scan
// in the same launch.
template <class FrP, int FUSED>
__global__ void __launch_bounds__(POLY_TPB) k_ratio_lanes(Fp<FrP> *va, Fp<FrP> *vb, size_t m, unsigned tb, Fp<FrP> *__restrict__ xa,
                                                          Fp<FrP> *__restrict__ xb, Fp<FrP> *__restrict__ sa, Fp<FrP> *__restrict__ sb) {
    using Fr = Fp<FrP>;
    __shared__ Fr la[POLY_TPB], lb[POLY_TPB];
    const unsigned l = threadIdx.x;
    const size_t g = (size_t)blockIdx.x * POLY_TPB + l;
    const size_t lo = g << tb, hi = min(lo + ((size_t)1 << tb), m);
    Fr a = Fr::one(), b = Fr::one();
#pragma nounroll
    for (size_t i = lo; i < hi; ++i) {
        a = fp_mul(a, fft_load(va, i));
        b = fp_mul(b, fft_load(vb, i));
    }
    la[l] = a;
    lb[l] = b;
    // prefix scan: after step j, (a, b) = the products over lanes l - 2^(j+1) + 1 .. l
#pragma nounroll
    for (unsigned j = 0; j < POLY_LOG_TPB; ++j) {
        const unsigned d = 1u << j;
        __syncthreads();
        const bool has = l >= d;
        Fr oa = Fr::one(), ob = Fr::one();
        if (has) oa = la[l - d], ob = lb[l - d];
        __syncthreads();
        if (has) a = fp_mul(a, oa), b = fp_mul(b, ob);
        la[l] = a;
        lb[l] = b;
    }
    if (!FUSED) {
        fft_store(xa, g, a);
        fft_store(xb, g, b);
        if (l == POLY_TPB - 1) {
            fft_store(sa, blockIdx.x, a);
            fft_store(sb, blockIdx.x, b);
        }
    } else {
        __syncthreads();
        const Fr ca = l > 0 ? la[l - 1] : Fr::one(), cb = l > 0 ? lb[l - 1] : Fr::one();
        ratio_lane_walk(va, vb, m, g, tb, ca, cb);
    }
}

// Pass 3: tile t = blockIdx.x, carries C_(t-1) from pass 2 (none below the first tile).
template <class FrP>
__global__ void __launch_bounds__(POLY_TPB) k_ratio_apply(Fp<FrP> *va, Fp<FrP> *vb, size_t m, unsigned tb, const Fp<FrP> *__restrict__ xa,
                                                          const Fp<FrP> *__restrict__ xb, const Fp<FrP> *__restrict__ ca,
                                                          const Fp<FrP> *__restrict__ cb) {
    using Fr = Fp<FrP>;
    const unsigned l = threadIdx.x;
    const size_t t = blockIdx.x, g = t * POLY_TPB + l;
    Fr ya = l > 0 ? fft_load(xa, g - 1) : Fr::one(), yb = l > 0 ? fft_load(xb, g - 1) : Fr::one();
    if (t > 0) {
        const Fr ta = fft_load(ca, t - 1), tb_ = fft_load(cb, t - 1);
        ya = l > 0 ? fp_mul(ya, ta) : ta;
        yb = l > 0 ? fp_mul(yb, tb_) : tb_;
    }
    ratio_lane_walk(va, vb, m, g, tb, ya, yb);
}

// Batch inversion with the zero rule, one workgroup = one tile of TPB lanes x T elements: out_i = 1/a_i (0 where a_i = 0),
// times mul_i when MUL. run: m elements of scratch (the running products). out may be a (and mul): a lane reads index i of
// every input before it writes index i, and never returns to it.
template <class FrP, int MUL>
__global__ void __launch_bounds__(POLY_TPB) k_ratio_invert(const Fp<FrP> *a, size_t m, unsigned tb, Fp<FrP> *__restrict__ run,
                                                           const Fp<FrP> *mul, Fp<FrP> *out) {
    using Fr = Fp<FrP>;
    __shared__ Fr tree[2 * POLY_TPB];  // node k = the product of nodes 2k and 2k + 1; the lanes are nodes TPB .. 2 TPB - 1
    const unsigned l = threadIdx.x;
    const size_t g = (size_t)blockIdx.x * POLY_TPB + l;
    const size_t lo = min(g << tb, m), hi = min(lo + ((size_t)1 << tb), m);
    Fr p = Fr::one();
#pragma nounroll
    for (size_t i = lo; i < hi; ++i) {
        const Fr x = fft_load(a, i);
        fft_store(run, i, p);
        if (!x.is_zero()) p = fp_mul(p, x);
    }
    tree[POLY_TPB + l] = p;
#pragma nounroll
    for (unsigned w = POLY_TPB / 2; w >= 1; w >>= 1) {
        __syncthreads();
        if (l < w) tree[w + l] = fp_mul(tree[2 * (w + l)], tree[2 * (w + l) + 1]);
    }
    __syncthreads();
    if (l == 0) tree[1] = fp_inv(tree[1]);  // never zero: zeros were skipped
    // down: node k holds the inverse of its product; its children get theirs
#pragma nounroll
    for (unsigned w = 1; w < POLY_TPB; w <<= 1) {
        __syncthreads();
        if (l < w) {
            const unsigned k = w + l;
            const Fr inv = tree[k], left = tree[2 * k], right = tree[2 * k + 1];
            tree[2 * k] = fp_mul(inv, right);
            tree[2 * k + 1] = fp_mul(inv, left);
        }
    }
    __syncthreads();
    Fr inv = tree[POLY_TPB + l];
#pragma nounroll
    for (size_t i = hi; i > lo; --i) {
        const Fr x = fft_load(a, i - 1);
        if (x.is_zero()) {
            fft_store(out, i - 1, Fr::zero());
            continue;
        }
        Fr r = fp_mul(inv, fft_load(run, i - 1));
        if (MUL) r = fp_mul(r, fft_load(mul, i - 1));
        fft_store(out, i - 1, r);
        inv = fp_mul(inv, x);
    }
}

// out <- z (n elements) unless the factor kernel found a permutation value out of range (*bad names its index): the last
// launch of a call whose permutation is on the device, so that a refused call writes nothing to its output
template <class FrP>
__global__ void __launch_bounds__(256) k_ratio_publish(const Fp<FrP> *__restrict__ z, Fp<FrP> *__restrict__ out, size_t n,
                                                       const unsigned long long *__restrict__ bad) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || *bad != ~0ull) return;
    fft_store(out, i, fft_load(z, i));
}

// ------------------------------------------------------------------ host side of one scalar field
template <class FrP>
struct RatioField {
    using Fr = Fp<FrP>;
    using PF = PolyField<FrP>;

    static size_t tiles(size_t m, unsigned lanes) {
        const size_t L = (size_t)POLY_TPB << PF::lane_bits(m, lanes);
        return (m + L - 1) / L;
    }
    // scratch elements scan2() needs for two vectors of m elements
    static size_t scan_scratch(size_t m, unsigned lanes) {
        const size_t nt = tiles(m, lanes);
        return nt <= 1 ? 0 : 2 * (nt * POLY_TPB + nt);
    }

    // va, vb (m >= 1 elements each, device) become their inclusive prefix products, on `stream`; lanes: the call's PF::lane_option()
    static int scan2(hipStream_t stream, Fr *va, Fr *vb, size_t m, Fr *scratch, unsigned lanes) {
        const unsigned tb = PF::lane_bits(m, lanes);
        const size_t nt = tiles(m, lanes);
        if (nt <= 1) {
            hipLaunchKernelGGL((k_ratio_lanes<FrP, 1>), dim3(1), dim3(POLY_TPB), 0, stream, va, vb, m, tb, nullptr, nullptr, nullptr, nullptr);
            HIP_TRY(hipGetLastError());
            return GMSM_OK;
        }
        Fr *xa = scratch, *xb = xa + nt * POLY_TPB, *sa = xb + nt * POLY_TPB, *sb = sa + nt;
        hipLaunchKernelGGL((k_ratio_lanes<FrP, 0>), dim3((unsigned)nt), dim3(POLY_TPB), 0, stream, va, vb, m, tb, xa, xb, sa, sb);
        // carries over the tile values, one workgroup; lanes of 2^tc tiles; in place
        unsigned tc = 0;
        while (((size_t)POLY_TPB << tc) < nt) ++tc;
        hipLaunchKernelGGL((k_ratio_lanes<FrP, 1>), dim3(1), dim3(POLY_TPB), 0, stream, sa, sb, nt, tc, nullptr, nullptr, nullptr, nullptr);
        hipLaunchKernelGGL((k_ratio_apply<FrP>), dim3((unsigned)nt), dim3(POLY_TPB), 0, stream, va, vb, m, tb, (const Fr *)xa, (const Fr *)xb,
                           (const Fr *)sa, (const Fr *)sb);
        HIP_TRY(hipGetLastError());
        return GMSM_OK;
    }

    // out_i = inv0(a_i) [mul_i], i < m (m >= 1); run: m elements of scratch; out may be a or mul
    static int invert(hipStream_t stream, const Fr *a, size_t m, Fr *run, const Fr *mul, Fr *out, unsigned lanes) {
        const unsigned tb = PF::lane_bits(m, lanes);
        const unsigned nt = (unsigned)tiles(m, lanes);
        if (mul) hipLaunchKernelGGL((k_ratio_invert<FrP, 1>), dim3(nt), dim3(POLY_TPB), 0, stream, a, m, tb, run, mul, out);
        else hipLaunchKernelGGL((k_ratio_invert<FrP, 0>), dim3(nt), dim3(POLY_TPB), 0, stream, a, m, tb, run, (const Fr *)nullptr, out);
        HIP_TRY(hipGetLastError());
        return GMSM_OK;
    }

    // bg[j] = beta g^j 2^-s, j < m (g = FrMultiplicativeGen, 2^s = the factor the domain's twiddles carry)
    static void coset_table(const FftDomain *d, const Fr &beta, size_t m, Fr *bg) {
        const Fr g = fr_from_limbs<Fr>(d->shift.data());
        Fr acc = fp_mul(beta, fp_inv(FftField<FrP>::lazy_shift()));
        for (size_t j = 0; j < m; ++j) {
            bg[j] = acc;
            acc = fp_mul(acc, g);
        }
    }

    // putInExpectedFormFromLagrangeRegular (ratios.go:248-273) on z (n = the domain's cardinality, Lagrange / Regular)
    static int expected_form(hipStream_t stream, FftDomain *d, Fr *z, int basis, uint32_t layout) {
        using FF = FftField<FrP>;
        const size_t n = (size_t)1 << d->log2n;
        int rc = GMSM_OK;
        if (basis != IOP_LAGRANGE) {
            std::lock_guard<std::mutex> lk(d->mu);
            if ((rc = FF::run(stream, d, z, /*inverse=*/true, /*dif=*/true, /*coset=*/false))) return rc;
            if (basis == IOP_LAGRANGE_COSET && (rc = FF::run(stream, d, z, false, /*dif=*/false, /*coset=*/true))) return rc;
        }
        const bool reverse = basis == IOP_CANONICAL ? layout == IOP_REGULAR : layout == IOP_BIT_REVERSE;
        return reverse ? FF::bit_reverse(stream, z, n) : rc;
    }
};

}  // namespace gmsm
