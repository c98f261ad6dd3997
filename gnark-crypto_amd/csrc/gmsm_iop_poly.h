// iop.Polynomial on the device: the basis changes, Evaluate and DivideByXMinusOne - what a PLONK prover does with a wire
// polynomial between the ratio entries (gmsm_ratio.h), the FFTs and the openings, without taking it back to the host.
//
// Replaces, with identical results (every output is a uniquely determined element of Fr, stored canonically in Montgomery
// form, so neither the order of a sum nor the way a vector is cut shows):
//   (*Polynomial).ToLagrange / ToCanonical / ToLagrangeCoset   ecc/bn254/fr/iop/polynomial.go:287-390 (with grow, :351-356)
//   (*Polynomial).Evaluate, (*polynomial).evaluate             polynomial.go:104-132, 198-261
//   (*Polynomial).GetCoeff                                     polynomial.go:151-163 (inside the quotient's gather)
//   DivideByXMinusOne, evaluateXnMinusOneDomainBigCoset        quotient.go:21-79
// and the twins of BLS12-381 and BW6-761 (same templates, other scalar fields).
//
// Departures from the reference, all of them here:
//   * Evaluate in a Lagrange basis at a point x of the domain gives 0, as the reference does (its prefactor x^len - 1 is
//     zero there and 1/0 = 0 in its batch inversion): reproduced, not repaired.
//   * A shift outside 0..5 is refused by the C entry; the reference multiplies x by an element it never initialised.
//   * A LagrangeCoset polynomial whose coset is 0 (it never went through ToLagrangeCoset) is evaluated at x 0^-1 = 0.
//
// Shape on the GPU, with no flag, spin or grid barrier between workgroups:
//   Basis changes   a zero-fill of [len, cardinality) on the stream (grow), then one or two transforms of gmsm_fft.h enqueued
//                   back to back: "leave the current basis" (FFTInverse, on the coset when the basis is LagrangeCoset), then
//                   "enter the target" (FFT, on the coset when the target is LagrangeCoset), each DIF from a Regular layout
//                   and DIT from a BitReverse one, each flipping the layout. That is the reference's switch, case by case.
//   Evaluate, Lagrange bases (the hot path), with w = fr.Generator(len):
//       value = (x^len - 1)/len * sum_i w^i c_i / (x - w^i)  and  w^i / (x - w^i) = x / (x - w^i) - 1,  so
//       value = (x^len - 1)/len * (x S1 - S0),  S1 = sum_i c_i / (x - w^i),  S0 = sum_i c_i
//     k_iop_bary         one pass over the coefficients, nothing of length len in HBM. A tile = 256 lanes x T = 2^tb indices:
//                        a lane's w^lo from the squarings w^(2^b) (k_fft_pow_table's method), then running products; the
//                        prefix products of its denominators x - w^i go to LDS; Montgomery's trick with ONE inversion per
//                        tile (the product tree of k_ratio_invert, zeros skipped: 1/0 = 0); the walk back (w^i by w^-1)
//                        leaves 1/(x - w^i) in the same LDS slots; then for each of the k polynomials one product per
//                        coefficient (bit-reversed read for BitReverse) and an LDS tree sum: two partials per tile and
//                        polynomial. The inverses are shared by the k polynomials.
//                        Products per coefficient: 2 up (w^i, prefix), 3 back (w^i, inverse, running inverse), k for the
//                        polynomials: 5 + k; per tile 3 * 255 + ~1.5 log2 q more.
//     k_iop_bary_finish  one workgroup per polynomial sums its partials and applies x and the prefactor.
//   Evaluate, Canonical   the suffix scan of gmsm_poly.h (evaluation only); BitReverse through its REV instantiation.
//   DivideByXMinusOne     k_iop_quotient_scale: out[bitrev(i)] = a[layout((i + rho shift) mod N)] inv[i mod rho], out of
//                         place (the input is never written), then FFTInverse(DIT, OnCoset) of the big domain in place on out.
//                         inv[j] = 1/(g^n t^j - 1), rho = N/n entries, built on the device for every rho (k_iop_xn_minus_one,
//                         then k_ratio_invert) and kept on the big domain per n, like its coset tables.
#pragma once
#include <hip/hip_runtime.h>
#include "gmsm_context.h"
#include "gmsm_field.h"
#include "gmsm_fft.h"
#include "gmsm_poly.h"
#include "gmsm_ratio.h"

namespace gmsm {

// indices per lane of k_iop_bary: at most 2^3 for a 32-byte element, 2^2 beyond (the tile's inverses live in LDS:
// 256 * T elements + the tree's 512)
template <class FrP>
constexpr unsigned iop_bary_max_lane_bits() { return sizeof(Fp<FrP>) <= 32 ? 3u : 2u; }

// Tile t = blockIdx.x of the barycentric sums at x over k polynomials of len = 2^log2len coefficients each (concatenated in
// polys, layouts[j] per polynomial). pw.p[b] = w^(2^b), w_inv = 1/w. part: 2 k nt elements; S1 of polynomial j and tile t at
// (2 j) nt + t, S0 at (2 j + 1) nt + t. Dynamic LDS: (256 * 2^tb + 512) elements.
template <class FrP>
__global__ void __launch_bounds__(POLY_TPB) k_iop_bary(const Fp<FrP> *__restrict__ polys, const uint32_t *__restrict__ layouts, size_t k,
                                                       size_t len, unsigned log2len, unsigned tb, FftPowers<FrP> pw, Fp<FrP> w_inv, Fp<FrP> x,
                                                       Fp<FrP> *__restrict__ part) {
    using Fr = Fp<FrP>;
    extern __shared__ __align__(16) unsigned char iop_lds_raw[];
    Fr *pre = reinterpret_cast<Fr *>(iop_lds_raw);  // [T][TPB]: slot (i - lo, lane)
    Fr *tree = pre + ((size_t)POLY_TPB << tb);      // node k = the product of nodes 2k and 2k + 1; the lanes are nodes TPB .. 2 TPB - 1
    const unsigned l = threadIdx.x;
    const size_t nt = gridDim.x, g = (size_t)blockIdx.x * POLY_TPB + l;
    const size_t lo = min(g << tb, len), hi = min(lo + ((size_t)1 << tb), len);
    Fr wi = Fr::one();  // w^lo
#pragma nounroll
    for (int b = 0; b < 40; ++b)
        if ((lo >> b) & 1) wi = fp_mul(wi, pw.p[b]);
    Fr p = Fr::one();
#pragma nounroll
    for (size_t i = lo; i < hi; ++i) {
        const Fr d = fp_sub(x, wi);
        pre[(i - lo) * POLY_TPB + l] = p;
        if (!d.is_zero()) p = fp_mul(p, d);
        wi = fp_mul(wi, pw.p[0]);
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
            const unsigned q = w + l;
            const Fr inv = tree[q], left = tree[2 * q], right = tree[2 * q + 1];
            tree[2 * q] = fp_mul(inv, right);
            tree[2 * q + 1] = fp_mul(inv, left);
        }
    }
    __syncthreads();
    Fr inv = tree[POLY_TPB + l];
    // back from w^hi: the slot of index i gets 1/(x - w^i), and 0 where x = w^i
#pragma nounroll
    for (size_t i = hi; i > lo; --i) {
        wi = fp_mul(wi, w_inv);
        const Fr d = fp_sub(x, wi);
        Fr r = Fr::zero();
        if (!d.is_zero()) {
            r = fp_mul(inv, pre[(i - 1 - lo) * POLY_TPB + l]);
            inv = fp_mul(inv, d);
        }
        pre[(i - 1 - lo) * POLY_TPB + l] = r;
    }
    // a lane reads its own slots only: no barrier between the walk and the sums
#pragma nounroll
    for (size_t j = 0; j < k; ++j) {
        const Fr *c = polys + j * len;
        const bool rev = layouts[j] == IOP_BIT_REVERSE;
        Fr s1 = Fr::zero(), s0 = Fr::zero();
#pragma nounroll
        for (size_t i = lo; i < hi; ++i) {
            const Fr v = fft_load(c, rev ? fft_bitrev(i, log2len) : i);
            s1 = fp_add(s1, fp_mul(v, pre[(i - lo) * POLY_TPB + l]));
            s0 = fp_add(s0, v);
        }
        __syncthreads();  // the tree's last readers (the inversion, or polynomial j - 1) are done
        tree[l] = s1;
        tree[POLY_TPB + l] = s0;
#pragma nounroll
        for (unsigned w = POLY_TPB / 2; w >= 1; w >>= 1) {
            __syncthreads();
            if (l < w) {
                tree[l] = fp_add(tree[l], tree[l + w]);
                tree[POLY_TPB + l] = fp_add(tree[POLY_TPB + l], tree[POLY_TPB + l + w]);
            }
        }
        if (l == 0) {  // lane 0 wrote both in the last step
            fft_store(part, (2 * j) * nt + blockIdx.x, tree[0]);
            fft_store(part, (2 * j + 1) * nt + blockIdx.x, tree[POLY_TPB]);
        }
    }
}

// Polynomial j = blockIdx.x: values[j] = pref (x S1 - S0) over the nt partials of k_iop_bary; pref = (x^len - 1)/len
template <class FrP>
__global__ void __launch_bounds__(POLY_TPB) k_iop_bary_finish(const Fp<FrP> *__restrict__ part, size_t nt, Fp<FrP> x, Fp<FrP> pref,
                                                              Fp<FrP> *__restrict__ values) {
    using Fr = Fp<FrP>;
    __shared__ Fr t1[POLY_TPB], t0[POLY_TPB];
    const unsigned l = threadIdx.x;
    const size_t j = blockIdx.x;
    Fr s1 = Fr::zero(), s0 = Fr::zero();
#pragma nounroll
    for (size_t s = l; s < nt; s += POLY_TPB) {
        s1 = fp_add(s1, fft_load(part, (2 * j) * nt + s));
        s0 = fp_add(s0, fft_load(part, (2 * j + 1) * nt + s));
    }
    t1[l] = s1;
    t0[l] = s0;
#pragma nounroll
    for (unsigned w = POLY_TPB / 2; w >= 1; w >>= 1) {
        __syncthreads();
        if (l < w) {
            t1[l] = fp_add(t1[l], t1[l + w]);
            t0[l] = fp_add(t0[l], t0[l + w]);
        }
    }
    if (l == 0) fft_store(values, j, fp_mul(pref, fp_sub(fp_mul(x, t1[0]), t0[0])));
}

// out[j] = scale base^j - 1, j < count, base^(2^b) = pw.p[b] (k_fft_pow_table's method): X^n - 1 on the big domain's coset,
// before its inversion (evaluateXnMinusOneDomainBigCoset, quotient.go:56-79)
template <class FrP>
__global__ void __launch_bounds__(256) k_iop_xn_minus_one(FftPowers<FrP> pw, Fp<FrP> scale, size_t count, Fp<FrP> *__restrict__ out) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count) return;
    Fp<FrP> acc = scale;
#pragma nounroll
    for (int b = 0; b < 40; ++b)
        if ((j >> b) & 1) acc = fp_mul(acc, pw.p[b]);
    fft_store(out, j, fp_sub(acc, Fp<FrP>::one()));
}

// The quotient's gather (quotient.go:40-47 with GetCoeff, polynomial.go:151-163). Lane o owns the OUTPUT position
// o = bitrev(i): out[o] = a[rev ? bitrev(s) : s] inv[i & rho_mask], s = (i + rs) mod N, rs = rho * shift mod N. a and out do
// not overlap (the entry refuses it).
template <class FrP>
__global__ void __launch_bounds__(256) k_iop_quotient_scale(const Fp<FrP> *__restrict__ a, size_t N, unsigned log2N, size_t rs, int rev,
                                                            const Fp<FrP> *__restrict__ inv, size_t rho_mask, Fp<FrP> *__restrict__ out) {
    const size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= N) return;
    const size_t i = fft_bitrev(o, log2N), s = (i + rs) & (N - 1);
    const Fp<FrP> c = fft_load(a, rev ? fft_bitrev(s, log2N) : s);
    fft_store(out, o, fp_mul(c, fft_load(inv, i & rho_mask)));
}

// ------------------------------------------------------------------ host side of one scalar field
template <class FrP>
struct IopPolyField {
    using Fr = Fp<FrP>;
    using PF = PolyField<FrP>;
    using FF = FftField<FrP>;
    using RF = RatioField<FrP>;

    // fr.Generator(2^log2n) (fr/generator.go:32-34); log2n <= MAX_ORDER (the entry has checked)
    static Fr generator(unsigned log2n) { return FF::pow2k(FF::from_words(FrP::ROOT_OF_UNITY), FrP::MAX_ORDER - log2n); }

    // The point the polynomial is really evaluated at (Evaluate, polynomial.go:106-125): x / coset for LagrangeCoset (0^-1 = 0),
    // then times Generator(size)^shift, shift in 1..5
    static Fr effective_point(const uint64_t *x, int basis, const uint64_t *coset, unsigned shift, size_t size) {
        Fr xx = fr_from_limbs<Fr>(x);
        if (basis == IOP_LAGRANGE_COSET) xx = fp_mul(xx, fp_inv(fr_from_limbs<Fr>(coset)));
        if (shift) {
            unsigned ls = 0;
            while (((size_t)1 << ls) < size) ++ls;
            const Fr g = generator(ls);
            for (unsigned s = 0; s < shift; ++s) xx = fp_mul(xx, g);
        }
        return xx;
    }

    // ---- the basis changes: the reference's switch as "leave the basis, enter the target"; the caller holds d->mu
    static int to_basis(hipStream_t stream, FftDomain *d, Fr *v, int basis, int layout, int target, int *out_layout) {
        bool regular = layout == (int)IOP_REGULAR;
        int rc = GMSM_OK;
        if (basis != target) {
            if (basis != IOP_CANONICAL) {
                if ((rc = FF::run(stream, d, v, /*inverse=*/true, /*dif=*/regular, /*coset=*/basis == IOP_LAGRANGE_COSET))) return rc;
                regular = !regular;
            }
            if (target != IOP_CANONICAL) {
                if ((rc = FF::run(stream, d, v, /*inverse=*/false, /*dif=*/regular, /*coset=*/target == IOP_LAGRANGE_COSET))) return rc;
                regular = !regular;
            }
        }
        *out_layout = regular ? (int)IOP_REGULAR : (int)IOP_BIT_REVERSE;
        return rc;
    }

    // ---- Evaluate in a Lagrange basis
    static unsigned bary_lane_bits(size_t len, unsigned lanes) { return std::min(PF::lane_bits(len, lanes), iop_bary_max_lane_bits<FrP>()); }
    static size_t bary_tiles(size_t len, unsigned lanes) {
        const size_t L = (size_t)POLY_TPB << bary_lane_bits(len, lanes);
        return (len + L - 1) / L;
    }
    static size_t bary_scratch(size_t k, size_t len, unsigned lanes) { return 2 * k * bary_tiles(len, lanes); }

    // values[j] (device) = polynomial j at x, j < k; polys: k * len elements (device), len = 2^log2len; layouts: k words (device);
    // part: bary_scratch(k, len, lanes) elements
    static int barycentric(hipStream_t stream, const Fr *polys, const uint32_t *layouts, size_t k, size_t len, unsigned log2len, const Fr &x,
                           Fr *part, Fr *values, unsigned lanes) {
        const unsigned tb = bary_lane_bits(len, lanes);
        const size_t nt = bary_tiles(len, lanes);
        const Fr w = generator(log2len);
        Fr xn = x, card = Fr::one();
        for (unsigned i = 0; i < log2len; ++i) xn = fp_sqr(xn), card = fp_dbl(card);
        const Fr pref = fp_mul(fp_sub(xn, Fr::one()), fp_inv(card));  // (x^len - 1) / len
        const size_t lds = (((size_t)POLY_TPB << tb) + 2 * POLY_TPB) * sizeof(Fr);
        if (int rc = ctx_allow_lds((const void *)k_iop_bary<FrP>, 128 * 1024)) return rc;
        hipLaunchKernelGGL((k_iop_bary<FrP>), dim3((unsigned)nt), dim3(POLY_TPB), lds, stream, polys, layouts, k, len, log2len, tb,
                           FF::powers_of(w), fp_inv(w), x, part);
        hipLaunchKernelGGL((k_iop_bary_finish<FrP>), dim3((unsigned)k), dim3(POLY_TPB), 0, stream, (const Fr *)part, nt, x, pref, values);
        HIP_TRY(hipGetLastError());
        return GMSM_OK;
    }

    // ---- Evaluate in Canonical basis: *value (device) = sum_i v[idx(i)] a^i, idx = bitrev when rev (m a power of two then);
    // scratch: PF::scratch_elems(m, lanes)
    static int eval_canonical(hipStream_t stream, const FftPowers<FrP> &pw, const Fr *v, size_t m, bool rev, Fr *value, Fr *scratch,
                              unsigned lanes) {
        if (!rev) return PF::suffix(stream, pw, v, m, nullptr, value, scratch, lanes);
        // PF::suffix's evaluation-only launches, the coefficients read through bitrev (the tile values of the second are in order)
        const unsigned tb = PF::lane_bits(m, lanes), logL = POLY_LOG_TPB + tb;
        const size_t L = (size_t)1 << logL, nt = (m + L - 1) / L;
        if (nt <= 1) {
            hipLaunchKernelGGL((k_poly_lanes<FrP, 1, 1>), dim3(1), dim3(POLY_TPB), 0, stream, v, m, pw, 0u, tb, nullptr, nullptr, nullptr, 1u, value);
            HIP_TRY(hipGetLastError());
            return GMSM_OK;
        }
        Fr *x = scratch, *s = x + nt * POLY_TPB, *c = s + nt;
        hipLaunchKernelGGL((k_poly_lanes<FrP, 0, 1>), dim3((unsigned)nt), dim3(POLY_TPB), 0, stream, v, m, pw, 0u, tb, x, s, nullptr, 0u, nullptr);
        unsigned tc = 0;
        while (((size_t)POLY_TPB << tc) < nt) ++tc;
        if (logL + tc + POLY_LOG_TPB > 39) return fail(GMSM_ERR_ARG, "polynomial too long for the carry pass");
        hipLaunchKernelGGL((k_poly_lanes<FrP, 1>), dim3(1), dim3(POLY_TPB), 0, stream, (const Fr *)s, nt, pw, logL, tc, nullptr, nullptr, c, 0u, value);
        HIP_TRY(hipGetLastError());
        return GMSM_OK;
    }

    // ---- DivideByXMinusOne
    // inv[j] = 1/(g^n t^j - 1), j < rho = N/n (g = the big domain's FrMultiplicativeGen, t = its Generator^n), resident on the big
    // domain per log2 n. Built on first use on `stream` and complete before the flag says so (any stream may read it next);
    // run: rho elements of scratch. The caller holds big->mu.
    static int ensure_xn_inv(hipStream_t stream, FftDomain *big, unsigned log2n, Fr *run, unsigned lanes, const Fr **table) {
        FftDomain::XnInv &e = big->xn_inv[log2n];
        if (!e.ready) {
            const size_t rho = (size_t)1 << (big->log2n - log2n);
            if (int rc = e.table.ensure(rho * sizeof(Fr))) return rc;
            const Fr g = fr_from_limbs<Fr>(big->shift.data()), w = fr_from_limbs<Fr>(big->generator.data());
            Fr *tbl = (Fr *)e.table.ptr;
            hipLaunchKernelGGL((k_iop_xn_minus_one<FrP>), dim3((unsigned)((rho + 255) / 256)), dim3(256), 0, stream, FF::powers_of(FF::pow2k(w, log2n)),
                               FF::pow2k(g, log2n), rho, tbl);
            if (int rc = RF::invert(stream, tbl, rho, run, nullptr, tbl, lanes)) return rc;
            HIP_TRY(hipStreamSynchronize(stream));
            e.ready = true;
        }
        *table = (const Fr *)e.table.ptr;
        return GMSM_OK;
    }

    // out (N elements, device, no overlap with a) <- the quotient in Canonical / Regular form; rs = rho * shift mod N. The
    // caller holds big->mu.
    static int quotient(hipStream_t stream, FftDomain *big, unsigned log2n, const Fr *a, bool rev, size_t rs, Fr *run, Fr *out, unsigned lanes) {
        const size_t N = (size_t)1 << big->log2n, rho = N >> log2n;
        const Fr *inv;
        int rc = ensure_xn_inv(stream, big, log2n, run, lanes, &inv);
        if (rc) return rc;
        hipLaunchKernelGGL((k_iop_quotient_scale<FrP>), dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream, a, N, big->log2n, rs, rev ? 1 : 0, inv,
                           rho - 1, out);
        HIP_TRY(hipGetLastError());
        return FF::run(stream, big, out, /*inverse=*/true, /*dif=*/false, /*coset=*/true);
    }
};

}  // namespace gmsm
