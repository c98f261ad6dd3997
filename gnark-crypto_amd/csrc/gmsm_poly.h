// KZG opening arithmetic on the device: the Horner evaluation and the division by (X - a) that kzg.Open and
// kzg.BatchOpenSinglePoint run on the host before they commit to the quotient.
//
// Replaces, with identical results (every output is a uniquely determined element of Fr, stored canonically in
// Montgomery form, so the order of evaluation does not show):
//   eval                    ecc/bn254/kzg/kzg.go:55-63     (sequential Horner)
//   dividePolyByXminusA     kzg.go:565-583                 (sequential synthetic division)
//   the gamma fold of BatchOpenSinglePoint                 kzg.go:302-320 (F = sum_i gamma^i f_i, f_i,j = 0 beyond len(f_i))
// and the twins of BLS12-381 and BW6-761 (same templates, other scalar fields).
//
// All of it is one linear recurrence run from the top: y_(n-1) = f_(n-1), y_i = f_i + a y_(i+1). Then f(a) = y_0 and the
// quotient is h_k = y_(k+1), k < n - 1 (the reference subtracts f(a) from f_0 and drops the remainder, so h does not
// depend on the claimed value). A suffix scan in three launches, with no flag, spin or grid barrier between workgroups:
//   1. k_poly_lanes   each lane runs Horner over T = 2^tb consecutive coefficients; the workgroup combines its lanes with
//                     a log-step scan in LDS (x_l += a^(T 2^j) x_(l + 2^j)) and writes every lane's in-tile suffix X_l and
//                     the tile's value S_t = X_0
//   2. k_poly_lanes   the same kernel, fused, in one workgroup over the nt tile values with base a^L (L = TPB T): the carry
//                     C_t = S_t + a^L C_(t+1)
//   3. k_poly_apply   each lane's carry-in X_(l+1) + a^(T (TPB-1-l)) C_(t+1) (the powers from one small table), then the
//                     walk down its T coefficients, writing h and y_0
// A vector of one tile runs as one launch (k_poly_lanes fused). Powers of a: FftPowers (p[b] = a^(2^b)); a scan in base
// a^(2^b0) reads p[b0 + .], so one array serves the coefficients and the tiles.
#pragma once
#include <hip/hip_runtime.h>
#include "gmsm_context.h"
#include "gmsm_field.h"
#include "gmsm_fft.h"

namespace gmsm {

constexpr unsigned POLY_TPB = 256;  // lanes per tile
constexpr unsigned POLY_LOG_TPB = 8;

// where coefficient i of a vector of m sits: i, or with REV its bit reversal (m a power of two: a BitReverse layout of package
// iop, gmsm_iop_poly.h)
template <int REV>
__device__ __forceinline__ size_t poly_index(size_t i, size_t m) {
    if (REV) return fft_bitrev(i, 63u - (unsigned)__clzll((unsigned long long)m));
    return i;
}

// Horner over lane g's coefficients [g T, g T + T) of v (zero beyond m), base p[b0]: sum_i v_i base^(i - g T)
template <class FrP, int REV = 0>
__device__ __forceinline__ Fp<FrP> poly_lane_horner(const Fp<FrP> *v, size_t m, size_t g, unsigned tb, const Fp<FrP> &base) {
    const size_t lo = g << tb, hi = min(lo + ((size_t)1 << tb), m);
    Fp<FrP> acc = Fp<FrP>::zero();
    if (lo < hi) {
        acc = fft_load(v, poly_index<REV>(hi - 1, m));
#pragma nounroll
        for (size_t i = hi - 1; i > lo; --i) acc = fp_add(fp_mul(acc, base), fft_load(v, poly_index<REV>(i - 1, m)));
    }
    return acc;
}

// The walk of lane g from its top coefficient down with carry-in y (the suffix value just above the lane): y_i = v_i + base y,
// y_i stored at out[i - shift] (shift 1: the quotient h; 0: the suffix values themselves); y_0 -> *value
template <class FrP, int REV = 0>
__device__ __forceinline__ void poly_lane_walk(const Fp<FrP> *v, size_t m, size_t g, unsigned tb, const Fp<FrP> &base, Fp<FrP> y,
                                               Fp<FrP> *out, unsigned shift, Fp<FrP> *value) {
    const size_t lo = g << tb, hi = min(lo + ((size_t)1 << tb), m);
#pragma nounroll
    for (size_t i = hi; i > lo; --i) {
        y = fp_add(fp_mul(y, base), fft_load(v, poly_index<REV>(i - 1, m)));
        if (out != nullptr && i - 1 >= shift) fft_store(out, i - 1 - shift, y);
    }
    if (lo == 0 && lo < hi && value != nullptr) fft_store(value, 0, y);
}

// Passes 1 and 2. One workgroup = one tile of TPB lanes x T coefficients. FUSED = 0: writes X_l (x_out, one per lane) and
// S_t (s_out, one per tile). FUSED = 1 (one tile, gridDim.x == 1): the walk follows the scan in the same launch. REV = 1 reads
// v in bit-reversed order (evaluation only: out is null).
template <class FrP, int FUSED, int REV = 0>
__global__ void __launch_bounds__(POLY_TPB) k_poly_lanes(const Fp<FrP> *__restrict__ v, size_t m, FftPowers<FrP> pw, unsigned b0,
                                                         unsigned tb, Fp<FrP> *__restrict__ x_out, Fp<FrP> *__restrict__ s_out,
                                                         Fp<FrP> *__restrict__ out, unsigned shift, Fp<FrP> *__restrict__ value) {
    using Fr = Fp<FrP>;
    __shared__ Fr lane[POLY_TPB];
    const unsigned l = threadIdx.x;
    const size_t g = (size_t)blockIdx.x * POLY_TPB + l;
    Fr x = poly_lane_horner<FrP, REV>(v, m, g, tb, pw.p[b0]);
    lane[l] = x;
    // suffix scan: after step j, x_l = sum over lanes l..l + 2^(j+1) - 1 of s_m a^(T (m - l))
#pragma nounroll
    for (unsigned j = 0; j < POLY_LOG_TPB; ++j) {
        const unsigned d = 1u << j;
        __syncthreads();
        Fr other = Fr::zero();
        const bool has = l + d < POLY_TPB;
        if (has) other = lane[l + d];
        __syncthreads();
        if (has) x = fp_add(x, fp_mul(other, pw.p[b0 + tb + j]));
        lane[l] = x;
    }
    if (!FUSED) {
        fft_store(x_out, g, x);
        if (l == 0) fft_store(s_out, blockIdx.x, x);
    } else {
        __syncthreads();
        const Fr cin = l + 1 < POLY_TPB ? lane[l + 1] : Fr::zero();
        poly_lane_walk<FrP, REV>(v, m, g, tb, pw.p[b0], cin, out, shift, value);
    }
}

// Pass 3: tile t = blockIdx.x, carry C_(t+1) from pass 2 (none above the last tile). apow[k] = a^(T k), k < TPB.
template <class FrP>
__global__ void __launch_bounds__(POLY_TPB) k_poly_apply(const Fp<FrP> *__restrict__ v, size_t m, Fp<FrP> base, unsigned tb,
                                                         const Fp<FrP> *__restrict__ x_in, const Fp<FrP> *__restrict__ carry,
                                                         size_t nt, const Fp<FrP> *__restrict__ apow, Fp<FrP> *__restrict__ out,
                                                         unsigned shift, Fp<FrP> *__restrict__ value) {
    using Fr = Fp<FrP>;
    const unsigned l = threadIdx.x;
    const size_t t = blockIdx.x, g = t * POLY_TPB + l;
    Fr cin = l + 1 < POLY_TPB ? fft_load(x_in, g + 1) : Fr::zero();
    if (t + 1 < nt) cin = fp_add(cin, fp_mul(fft_load(apow, POLY_TPB - 1 - l), fft_load(carry, t + 1)));
    poly_lane_walk(v, m, g, tb, base, cin, out, shift, value);
}

// F_j = sum_i gamma^i f_(i,j) for j < maxlen (Horner in gamma over the k polynomials; f_(i,j) = 0 for j >= len_i).
// off_len: k pairs (offset of polynomial i in polys, its length), in elements.
template <class FrP>
__global__ void __launch_bounds__(256) k_poly_fold(const Fp<FrP> *__restrict__ polys, const uint64_t *__restrict__ off_len, size_t k,
                                                   size_t maxlen, Fp<FrP> gamma, Fp<FrP> *__restrict__ folded) {
    using Fr = Fp<FrP>;
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= maxlen) return;
    Fr acc = Fr::zero();
#pragma nounroll
    for (size_t i = k; i-- > 0;) {
        acc = fp_mul(acc, gamma);
        if (j < off_len[2 * i + 1]) acc = fp_add(acc, fft_load(polys, off_len[2 * i] + j));
    }
    fft_store(folded, j, acc);
}

// ------------------------------------------------------------------ host side of one scalar field
template <class FrP>
struct PolyField {
    using Fr = Fp<FrP>;

    // lane width 2^tb by length: long vectors take long lanes (the scan's ~7 products per lane are spread over more
    // coefficients), short ones short lanes (more lanes in flight)
    // GMSM_OPT_POLY_LANE_BITS (lanes = k in 1..6) forces 2^(k-1) for every length: the tests reach the carry pass's lanes of
    // several tiles, and every lane width on ragged tiles, at lengths a big-int model handles
    static unsigned lane_bits(size_t m, unsigned lanes) {
        if (lanes) return lanes - 1;
        return m > ((size_t)1 << 18) ? 5u : m > ((size_t)1 << 14) ? 4u : 3u;
    }
    // The switch, read ONCE per ABI call: the caller hands the same value to scratch_elems and to suffix, so the scratch a call
    // sized and the launches it makes agree even when another thread sets the switch meanwhile.
    static unsigned lane_option() { return options().poly_lane_bits.load(std::memory_order_relaxed); }

    // scratch elements suffix() needs for a vector of m coefficients
    static size_t scratch_elems(size_t m, unsigned lanes) {
        const unsigned tb = lane_bits(m, lanes);
        const size_t L = (size_t)POLY_TPB << tb, nt = (m + L - 1) / L;
        return nt <= 1 ? 0 : nt * POLY_TPB + 2 * nt + POLY_TPB;
    }

    // The suffix recurrence over v (m >= 1 coefficients, device) at the point whose powers are pw, on `stream`:
    // h (m - 1 elements, may be null) and y_0 = f(a) (*value, device, may be null). scratch: scratch_elems(m, lanes) elements,
    // lanes: the call's lane_option().
    static int suffix(hipStream_t stream, const FftPowers<FrP> &pw, const Fr *v, size_t m, Fr *h, Fr *value, Fr *scratch, unsigned lanes) {
        const unsigned tb = lane_bits(m, lanes), logL = POLY_LOG_TPB + tb;
        const size_t L = (size_t)1 << logL, nt = (m + L - 1) / L;
        if (nt <= 1) {
            hipLaunchKernelGGL((k_poly_lanes<FrP, 1>), dim3(1), dim3(POLY_TPB), 0, stream, v, m, pw, 0u, tb, nullptr, nullptr, h, 1u, value);
            HIP_TRY(hipGetLastError());
            return GMSM_OK;
        }
        Fr *x = scratch, *s = x + nt * POLY_TPB, *c = s + nt, *apow = c + nt;
        hipLaunchKernelGGL((k_poly_lanes<FrP, 0>), dim3((unsigned)nt), dim3(POLY_TPB), 0, stream, v, m, pw, 0u, tb, x, s, nullptr, 0u, nullptr);
        // carries over the tile values in base a^L, one workgroup; lanes of 2^tc tiles
        unsigned tc = 0;
        while (((size_t)POLY_TPB << tc) < nt) ++tc;
        if (logL + tc + POLY_LOG_TPB > 39) return fail(GMSM_ERR_ARG, "polynomial too long for the carry pass");
        const bool eval_only = h == nullptr;
        hipLaunchKernelGGL((k_poly_lanes<FrP, 1>), dim3(1), dim3(POLY_TPB), 0, stream, (const Fr *)s, nt, pw, logL, tc, nullptr, nullptr, c, 0u,
                           eval_only ? value : nullptr);
        if (!eval_only) {
            // a^(T k), k < TPB: k_fft_pow_table over the powers of a^T
            FftPowers<FrP> pt;
            for (int b = 0; b < 40; ++b) pt.p[b] = b + tb < 40 ? pw.p[b + tb] : Fr::zero();
            hipLaunchKernelGGL((k_fft_pow_table<FrP>), dim3(1), dim3(POLY_TPB), 0, stream, pt, Fr::one(), (size_t)POLY_TPB, apow, 0u);
            hipLaunchKernelGGL((k_poly_apply<FrP>), dim3((unsigned)nt), dim3(POLY_TPB), 0, stream, v, m, pw.p[0], tb, (const Fr *)x,
                               (const Fr *)c, nt, (const Fr *)apow, h, 1u, value);
        }
        HIP_TRY(hipGetLastError());
        return GMSM_OK;
    }

    static FftPowers<FrP> powers_of(const uint64_t *point) { return FftField<FrP>::powers_of(fr_from_limbs<Fr>(point)); }

    // F = sum_i gamma^i f_i (maxlen elements, device) from k polynomials concatenated in polys (lens[i] elements each);
    // off_len: 2k uint64 of device scratch
    static int fold(hipStream_t stream, const Fr *polys, const size_t *lens, size_t k, size_t maxlen, const uint64_t *gamma,
                    uint64_t *off_len, Fr *folded) {
        std::vector<uint64_t> ol(2 * k);
        size_t off = 0;
        for (size_t i = 0; i < k; ++i) ol[2 * i] = off, ol[2 * i + 1] = lens[i], off += lens[i];
        HIP_TRY(hipMemcpyAsync(off_len, ol.data(), ol.size() * 8, hipMemcpyHostToDevice, stream));
        HIP_TRY(hipStreamSynchronize(stream));  // `ol` is pageable host memory that goes out of scope
        hipLaunchKernelGGL((k_poly_fold<FrP>), dim3((unsigned)((maxlen + 255) / 256)), dim3(256), 0, stream, polys, (const uint64_t *)off_len, k,
                           maxlen, fr_from_limbs<Fr>(gamma), folded);
        HIP_TRY(hipGetLastError());
        return GMSM_OK;
    }
};

}  // namespace gmsm
