// The opening pipeline of shplonk.BatchOpen and fflonk.BatchOpen, and fflonk's Fold and FoldAndCommit
// (ecc/<curve>/fflonk/fflonk.go:41-141). A pack of polynomials P_0 .. P_(c-1) is interleaved into F = Fold(pack) =
// sum_(j<t) P_j(X^t) X^j, t = the smallest divisor of r - 1 that is >= c (P_j = 0 for c <= j < t), and F is opened by
// shplonk.BatchOpen on the orbit {z, wz, .., w^(t-1) z} of every base point z, w = g^((r-1)/t). The reference folds on the
// host, evaluates every P_j at every z^t, and runs shplonk over vectors t times longer with sets t times larger. The fold
// has structure that shplonk's chain of divisions (derived in gmsm_shplonk.h) does not see:
//   the orbit of z_k has the vanishing polynomial X^t - a_k, a_k = z_k^t, so Z_(ext S) = prod_k (X^t - a_k);
//   dividing F by X^t - a is t independent divisions of the P_j by (Y - a), interleaved again, hence
//   F div Z_(ext S) = Fold(P_j div prod_k (Y - a_k)).
// So w = sum_i gamma^i Fold_i(q_(i,j)) with q_(i,j) the quotient of member j of pack i by its pack's prod_k (Y - a_k): t_i
// chains of m_i suffix scans (PolyField::suffix) over n_i coefficients on the polynomials as given, instead of one chain of
// t_i m_i scans over t_i n_i coefficients. The folded vector is never formed for w: k_open_accumulate adds gamma^i q into
// the residue class j of w. The remainders of member j's chain are the Newton coefficients of its interpolant on {a_k}, so
// the outer claimed values P_j(a_k) (fflonk.go:104-116) are ShplonkField::claimed_from_remainders, and the inner (shplonk)
// claimed values F(w^l z_k) = sum_j (w^l z_k)^j P_j(a_k) - the sum BatchVerify recomputes (fflonk.go:180-191) - are
// O(t^2 m) host operations. L = sum_i c_i F_i - c_w w - const reads F_i from the pack in place (k_open_combine); its
// scalars are ShplonkField::combine_coefficients over the extended sets.
// shplonk.BatchOpen itself is the same opening with every polynomial a pack of its own: t_i = 1, a_k = z_k, the extended
// set the set, F_i = f_i, and gmsm_shplonk.h's formulation is what is left. One plan (FflonkField::Plan, built from packs
// or in that singleton form), one chains() and one combine() serve both families of entries.
// Every output is a uniquely determined element of Fr in canonical Montgomery form, so the results are the reference's bit
// for bit. Launches only: no flag, spin or grid barrier between workgroups.
#pragma once
#include <string>
#include <vector>
#include "gmsm_shplonk.h"

namespace gmsm {

// out[j t + i] = p_i[j] for i < count, j < len_i, zero elsewhere; o < total = t max_i len_i. One thread per output, so the
// writes are coalesced and a wave reads ~64/t consecutive coefficients of each member.
// off_len: count pairs (offset of member i in polys, its length), in elements.
template <class FrP>
__global__ void __launch_bounds__(256) k_fflonk_fold(const Fp<FrP> *__restrict__ polys, const uint64_t *__restrict__ off_len, size_t count,
                                                     size_t t, size_t total, Fp<FrP> *__restrict__ out) {
    using Fr = Fp<FrP>;
    const size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= total) return;
    const size_t j = o / t, i = o - j * t;
    Fr v = Fr::zero();
    if (i < count && j < off_len[2 * i + 1]) v = fft_load(polys, off_len[2 * i] + j);
    fft_store(out, o, v);
}

// w[e t + j] += c q[e] for e < n: gamma^i times one member's quotient into its residue class of w (w is zero-filled
// beforehand; t = 1, j = 0: w += c q)
template <class FrP>
__global__ void __launch_bounds__(256) k_open_accumulate(Fp<FrP> *__restrict__ w, const Fp<FrP> *__restrict__ q, size_t n, size_t t, size_t j,
                                                           Fp<FrP> c) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const size_t at = e * t + j;
    fft_store(w, at, fp_add(fft_load(w, at), fp_mul(fft_load(q, e), c)));
}

// L_e = sum_i c_i F_i[e] - c_w w_e for e < maxlen, less the constant at e = 0. F_i[e] is read from pack i in place: member
// e mod t_i, coefficient e div t_i, zero past the member's length or the pack's size. t_i is uniform over the wave, and a
// pack of one (all of them for shplonk) skips the 64-bit division.
// off_len: one pair per polynomial of all packs; packs: k triples (t_i, index of the first member, member count);
// coef: c_0 .. c_(k-1), c_w, the constant.
template <class FrP>
__global__ void __launch_bounds__(256) k_open_combine(const Fp<FrP> *__restrict__ polys, const uint64_t *__restrict__ off_len,
                                                        const uint64_t *__restrict__ packs, size_t k, size_t maxlen,
                                                        const Fp<FrP> *__restrict__ coef, const Fp<FrP> *__restrict__ w, Fp<FrP> *__restrict__ out) {
    using Fr = Fp<FrP>;
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= maxlen) return;
    Fr acc = fp_neg(fp_mul(fft_load(w, e), fft_load(coef, k)));
#pragma nounroll
    for (size_t i = 0; i < k; ++i) {
        const uint64_t t = packs[3 * i];
        uint64_t d = e, j = 0;
        if (t != 1) d = e / t, j = e - d * t;
        if (j >= packs[3 * i + 2]) continue;
        const uint64_t m = packs[3 * i + 1] + j;
        if (d < off_len[2 * m + 1]) acc = fp_add(acc, fp_mul(fft_load(polys, off_len[2 * m] + d), fft_load(coef, i)));
    }
    if (e == 0) acc = fp_sub(acc, fft_load(coef, k + 1));
    fft_store(out, e, acc);
}

// ------------------------------------------------------------------ host side of one scalar field
static const char *const ERR_FFLONK_SIZE = "invalid polynomial size (larger than SRS or == 0)";  // ErrInvalidPolynomialSize, kzg.go

template <class FrP>
struct FflonkField {
    using Fr = Fp<FrP>;
    using PF = PolyField<FrP>;
    using SF = ShplonkField<FrP>;

    // (r - 1) mod i and (r - 1) div i for a 64-bit i > 0 (quotient: FrP::N words, may be null)
    static uint64_t r_minus_one_divmod(uint64_t i, uint32_t *quot) {
        unsigned __int128 rem = 0;
        for (int l = FrP::N - 1; l >= 0; --l) {
            const uint32_t word = l == 0 ? FrP::Q[0] - 1 : FrP::Q[l];  // r is odd: no borrow
            rem = (rem << 32) | word;
            if (quot) quot[l] = (uint32_t)(rem / i);
            rem %= i;
        }
        return (uint64_t)rem;
    }
    // getNextDivisorRMinusOne (fflonk.go:234-252): the smallest divisor of r - 1 that is >= n, within 100 trials (the
    // reference panics when its counter reaches zero, which includes a divisor met at the hundredth step)
    static bool next_divisor(size_t n, size_t *t) {
        if (n == 0) return false;
        uint64_t i = n;
        int trials = 100;
        while (r_minus_one_divmod(i, nullptr) != 0 && trials > 0) {
            if (++i == 0) return false;
            --trials;
        }
        if (trials == 0) return false;
        *t = (size_t)i;
        return true;
    }
    static Fr pow_u64(Fr x, uint64_t e) {
        Fr acc = Fr::one();
        for (; e; e >>= 1, x = fp_sqr(x))
            if (e & 1) acc = fp_mul(acc, x);
        return acc;
    }
    // getIthRootOne (fflonk.go:213-230) for t | r - 1: g^((r-1)/t), g = fft.GeneratorFullMultiplicativeGroup()
    static Fr root_of_one(size_t t) {
        uint32_t e[FrP::N];
        r_minus_one_divmod(t, e);
        Fr acc = Fr::one();
        const Fr g = FftField<FrP>::from_words(FrP::MULT_GEN);
        for (int b = 32 * FrP::N - 1; b >= 0; --b) {
            acc = fp_sqr(acc);
            if ((e[b / 32] >> (b % 32)) & 1) acc = fp_mul(acc, g);
        }
        return acc;
    }

    // What a call derives from its arguments on the host, before any device work: groups of polynomials (fflonk's packs, or
    // every polynomial on its own for shplonk) that share a divisor t and a set of m points.
    struct Plan {
        bool single = false;                   // shplonk's singleton form: every t = 1, every count = 1
        size_t k = 0, npolys = 0, total = 0;  // groups, polynomials, coefficients of all polynomials
        size_t np = 0, nrem = 0, next = 0;     // sum m_i; sum count_i m_i (chain remainders); sum t_i m_i (extended points)
        size_t nclaimed = 0;                   // sum t_i m_i as well: t_i rows of m_i outer claimed values
        size_t maxfold = 0, maxmember = 0;     // max_i t_i n_i; the longest polynomial
        size_t wlen = 0;                       // true length of w
        std::vector<size_t> t, n, first, count, m;
        std::vector<size_t> member_points;     // m of its group, per polynomial
        std::vector<Fr> a, a_members;          // a_k = z_k^t_i in the layout of points; the same sets once per polynomial
        std::vector<Fr> ext;                   // extendSet (fflonk.go:255-271): [k t + l] = z_k w^l, group after group
        std::vector<size_t> ext_npoints;       // t_i m_i
        size_t table_words() const { return 2 * npolys + 3 * k; }  // what tables() writes
    };

    // From packs - alone (points == null: Fold) or with their points - or, with pack_sizes == null, in singleton form:
    // polynomial i is group i, t = 1, a = the points as given and the extended set is the set itself, so no divisor, root of
    // one or power is computed and the host cost is O(sum m_i) plus the comparison of the points. The two forms word and
    // order the refusals of a group as their references do. E: the entry's name for the texts.
    static int plan(const char *E, const size_t *lens, const size_t *pack_sizes, size_t k, const uint64_t *points, const size_t *npoints,
                    bool check_size, size_t registered, Plan *out) {
        Plan &p = *out;
        p = Plan();
        p.k = k, p.single = !pack_sizes;
        const std::string e(E);
        auto refuse = [&](const char *what, size_t i, const std::string &why) {
            return fail(GMSM_ERR_ARG, e + ": " + what + " " + std::to_string(i) + why);
        };
        for (size_t i = 0; i < k; ++i) {
            const size_t count = p.single ? 1 : pack_sizes[i];
            const bool no_point = points && npoints[i] == 0;
            size_t t = 1;
            if (!p.single) {
                if (count == 0) return refuse("pack", i, " holds no polynomial");
                if (no_point) return refuse("pack", i, " has no opening point");
                if (!next_divisor(count, &t))
                    return refuse("pack", i, ": did not find any divisor of r-1 within 100 trials above " + std::to_string(count));
            }
            size_t n = 0;
            for (size_t j = 0; j < count; ++j) {
                const size_t len = lens[p.npolys + j];
                n = std::max(n, len), p.total += len;
            }
            if (n == 0) return refuse("polynomial", i, " is empty (eval reads p[len(p)-1])");
            if (p.single && no_point) return refuse("polynomial", i, " has no opening point");
            if (!p.single && n > (~(size_t)0 >> 1) / t) return fail(GMSM_ERR_ARG, ERR_FFLONK_SIZE);
            p.t.push_back(t), p.n.push_back(n), p.first.push_back(p.npolys), p.count.push_back(count);
            p.m.push_back(points ? npoints[i] : 0);
            p.npolys += count;
            p.maxfold = std::max(p.maxfold, t * n), p.maxmember = std::max(p.maxmember, n);
        }
        if (!points) return GMSM_OK;
        const Fr *pts = (const Fr *)points;
        size_t max_size = p.maxfold;
        for (size_t i = 0, at = 0; i < k; at += p.m[i], ++i) {
            const size_t t = p.t[i], m = p.m[i];
            const size_t e0 = p.ext.size();
            if (p.single) {
                p.a.insert(p.a.end(), pts + at, pts + at + m);
                p.ext.insert(p.ext.end(), pts + at, pts + at + m);
            } else {
                const Fr omega = root_of_one(t);
                for (size_t c = 0; c < m; ++c) {
                    Fr x = pts[at + c];
                    p.a.push_back(pow_u64(x, t));
                    for (size_t l = 0; l < t; ++l, x = fp_mul(x, omega)) p.ext.push_back(x);
                }
            }
            // two equal points in an extended set (z_a = z_b, z_a^t = z_b^t, or z = 0 with t > 1): shplonk's interpolate inverts
            // zero there (shplonk.go:406-415) and returns a meaningless proof without an error. == compares the limbs as they are.
            for (size_t x = 0; x < t * m; ++x)
                for (size_t y = x + 1; y < t * m; ++y)
                    if (p.ext[e0 + x] == p.ext[e0 + y])
                        return fail(GMSM_ERR_ARG, e + ": set " + std::to_string(i) + " holds the same point twice (points " + std::to_string(x) +
                                                      " and " + std::to_string(y) + ")");
            p.ext_npoints.push_back(t * m);
            p.np += m, p.next += t * m, p.nrem += p.count[i] * m;
            max_size = std::max(max_size, t * m + 1);
            for (size_t j = 0; j < p.count[i]; ++j) {
                const size_t len = lens[p.first[i] + j];
                p.member_points.push_back(m);
                p.a_members.insert(p.a_members.end(), p.a.begin() + at, p.a.begin() + at + m);
                if (len > m) p.wlen = std::max(p.wlen, (len - m - 1) * t + j + 1);
            }
        }
        p.nclaimed = p.next;
        // shplonk's size condition over the folded sizes (shplonk.go:66-83, :163-166)
        if (check_size && max_size + p.next - 1 > registered) return fail(GMSM_ERR_ARG, ERR_FFLONK_SIZE);
        return GMSM_OK;
    }

    // (offset, length) pairs of the polynomials, then (t, first member, member count) per group: table_words() words
    static void tables(const Plan &p, const size_t *lens, uint64_t *out) {
        size_t off = 0;
        for (size_t j = 0; j < p.npolys; off += lens[j], ++j) out[2 * j] = off, out[2 * j + 1] = lens[j];
        uint64_t *packs = out + 2 * p.npolys;
        for (size_t i = 0; i < p.k; ++i) packs[3 * i] = p.t[i], packs[3 * i + 1] = p.first[i], packs[3 * i + 2] = p.count[i];
    }

    static int fold(hipStream_t stream, const Fr *polys, const uint64_t *off_len, size_t count, size_t t, size_t total, Fr *out) {
        hipLaunchKernelGGL((k_fflonk_fold<FrP>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, polys, off_len, count, t, total,
                           out);
        HIP_TRY(hipGetLastError());
        return GMSM_OK;
    }

    // The chains and the accumulation on `stream`: rem (nrem elements, device) receives the remainders, member after member
    // (m_i each); w (maxfold elements, device) sum_i gamma^i Fold_i(q_(i,j)). a, b: ping-pong vectors of maxmember - 1
    // elements; scratch: ShplonkField::chain_scratch over (lens, member_points) for the same lanes.
    static int chains(hipStream_t stream, const Plan &p, const Fr *polys, const size_t *lens, const Fr &gamma, Fr *rem, Fr *w, Fr *a, Fr *b,
                      Fr *scratch, unsigned lanes) {
        HIP_TRY(hipMemsetAsync(rem, 0, p.nrem * sizeof(Fr), stream));  // a chain that runs out of coefficients leaves d = 0
        HIP_TRY(hipMemsetAsync(w, 0, p.maxfold * sizeof(Fr), stream));
        Fr acc_gamma = Fr::one();
        int rc;
        size_t off = 0, r = 0;
        for (size_t i = 0, at = 0; i < p.k; at += p.m[i], ++i) {
            for (size_t j = 0; j < p.count[i]; off += lens[p.first[i] + j], r += p.m[i], ++j) {
                const Fr *cur = polys + off;
                size_t n = lens[p.first[i] + j];
                for (size_t c = 0; c < p.m[i] && n > 0; ++c, --n) {
                    Fr *dst = (c & 1) ? b : a;
                    if ((rc = PF::suffix(stream, FftField<FrP>::powers_of(p.a[at + c]), cur, n, n > 1 ? dst : nullptr, rem + r + c, scratch, lanes)))
                        return rc;
                    cur = dst;
                }
                if (n > 0) {
                    hipLaunchKernelGGL((k_open_accumulate<FrP>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, w, cur, n, p.t[i], j,
                                       acc_gamma);
                    HIP_TRY(hipGetLastError());
                }
            }
            acc_gamma = fp_mul(acc_gamma, gamma);
        }
        return GMSM_OK;
    }

    // From the chains' remainders (host copy): claimed = ClaimedValues[i][j][k], pack after pack t_i rows of m_i values with
    // the rows j >= count_i zero; folded = SOpeningProof.ClaimedValues[i][k t_i + l] = sum_j (w^l z_k)^j P_j(a_k).
    // Singleton form: claimed is the values in the layout of points, folded is not written (may be null).
    static void claimed_values(const Plan &p, const Fr *rem, Fr *claimed, Fr *folded) {
        if (p.single) {
            SF::claimed_from_remainders(p.a.data(), p.m.data(), p.k, rem, claimed);
            return;
        }
        std::vector<Fr> inner(p.nrem);
        SF::claimed_from_remainders(p.a_members.data(), p.member_points.data(), p.npolys, rem, inner.data());
        for (size_t i = 0, r = 0, o = 0; i < p.k; r += p.count[i] * p.m[i], o += p.t[i] * p.m[i], ++i) {
            const size_t t = p.t[i], m = p.m[i], c = p.count[i];
            for (size_t x = 0; x < t * m; ++x) claimed[o + x] = x < c * m ? inner[r + x] : Fr::zero();
            for (size_t q = 0; q < m; ++q)
                for (size_t l = 0; l < t; ++l) {
                    const Fr &x = p.ext[o + q * t + l];
                    Fr acc = Fr::zero();
                    for (size_t j = c; j-- > 0;) acc = fp_add(fp_mul(acc, x), inner[r + j * m + q]);
                    folded[o + q * t + l] = acc;
                }
        }
    }

    static int combine(hipStream_t stream, const Plan &p, const Fr *polys, const uint64_t *tables, const Fr *coef, const Fr *w, Fr *out) {
        hipLaunchKernelGGL((k_open_combine<FrP>), dim3((unsigned)((p.maxfold + 255) / 256)), dim3(256), 0, stream, polys, tables,
                           tables + 2 * p.npolys, p.k, p.maxfold, coef, w, out);
        HIP_TRY(hipGetLastError());
        return GMSM_OK;
    }
};

}  // namespace gmsm
