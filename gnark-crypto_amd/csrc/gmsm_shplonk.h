// shplonk.BatchOpen (ecc/<curve>/shplonk/shplonk.go:44-172): polynomial i is opened on its own set of points S_i (m_i of
// them), T = the concatenation of the sets. The reference forms, over full-length vectors on the host,
//   w  = (sum_i gamma^i Z_(T\S_i) (f_i - r_i)) / Z_T            r_i = the interpolant of f_i on S_i   (:97-120)
//   w' = (sum_i c_i (f_i - r_i(z)) - Z_T(z) w) / (X - z)        c_i = gamma^i Z_(T\S_i)(z)            (:132-164)
// with a naive product by Z_(T\S_i) and a naive division by Z_T. The same results without those products:
//   Z_T = Z_(T\S_i) Z_(S_i), so w = sum_i gamma^i q_i with q_i the polynomial quotient of f_i by Z_(S_i) (deg r_i < m_i:
//   subtracting r_i only removes the remainder). q_i is a chain of m_i divisions by (X - s_(i,j)), each one suffix scan
//   (PolyField::suffix): q_(i,0) = f_i, q_(i,j) = q_(i,j-1) div (X - s_(i,j)). The chain's remainders d_(i,j) =
//   q_(i,j-1)(s_(i,j)) are the Newton coefficients of r_i = d_1 + d_2 (X - s_1) + d_3 (X - s_1)(X - s_2) + ..., so the
//   claimed values f_i(s_(i,j)) = r_i(s_(i,j)) are a host evaluation of that form: no further pass over f_i.
//   L = sum_i c_i f_i - (sum_i c_i r_i(z)) - Z_T(z) w in one pass, w' = L div (X - z) in one scan.
// This header holds the host arithmetic of that formulation: the scalars that depend on the points only (gamma^i,
// Z_(T\S_i)(z), Z_T(z), r_i(z), the claimed values), O((sum_i m_i)^2) field operations, none of which touches a coefficient
// vector. The device part - chains, accumulation, L - is the opening pipeline of gmsm_fflonk.h, which shplonk enters as
// the opening whose packs hold one polynomial each (t_i = 1).
#pragma once
#include <vector>
#include "gmsm_poly.h"

namespace gmsm {

// ------------------------------------------------------------------ host side of one scalar field
template <class FrP>
struct ShplonkField {
    using Fr = Fp<FrP>;
    using PF = PolyField<FrP>;

    // d_1 + (x - s_1)(d_2 + (x - s_2)(d_3 + ...)): the Newton form with coefficients d on the nodes s
    static Fr newton_eval(const Fr *s, const Fr *d, size_t m, const Fr &x) {
        Fr acc = d[m - 1];
        for (size_t j = m - 1; j-- > 0;) acc = fp_add(fp_mul(acc, fp_sub(x, s[j])), d[j]);
        return acc;
    }
    // the Newton coefficients of the interpolant of (s_j, y_j): divided differences, in place over d = y (nodes distinct)
    static void newton_from_values(const Fr *s, Fr *d, size_t m) {
        for (size_t l = 1; l < m; ++l)
            for (size_t j = m - 1; j >= l; --j) d[j] = fp_mul(fp_sub(d[j], d[j - 1]), fp_inv(fp_sub(s[j], s[j - l])));
    }

    // scratch PolyField::suffix needs along the chain of polynomial lengths len, len - 1, ... (lane widths change with the length)
    static size_t chain_scratch(const size_t *lens, const size_t *npoints, size_t k, unsigned lanes) {
        size_t s = 0;
        for (size_t i = 0; i < k; ++i)
            for (size_t j = 0; j < npoints[i] && j < lens[i]; ++j) s = std::max(s, PF::scratch_elems(lens[i] - j, lanes));
        return s;
    }

    // claimed values f_i(s_(i,j)) from the chain's remainders (both sum_i m_i elements, the layout of points)
    static void claimed_from_remainders(const Fr *points, const size_t *npoints, size_t k, const Fr *rem, Fr *claimed) {
        for (size_t i = 0, p = 0; i < k; p += npoints[i], ++i)
            for (size_t j = 0; j < npoints[i]; ++j) claimed[p + j] = newton_eval(points + p, rem + p, j + 1, points[p + j]);
    }

    // coef (k + 2 elements): c_i = gamma^i Z_(T\S_i)(z), then Z_T(z), then sum_i c_i r_i(z)
    static void combine_coefficients(const Fr *points, const size_t *npoints, size_t k, const Fr *claimed, const Fr &gamma, const Fr &z,
                                     Fr *coef) {
        std::vector<Fr> zs(k);  // Z_(S_i)(z)
        size_t maxm = 0;
        for (size_t i = 0, p = 0; i < k; p += npoints[i], ++i) {
            Fr v = Fr::one();
            for (size_t j = 0; j < npoints[i]; ++j) v = fp_mul(v, fp_sub(z, points[p + j]));
            zs[i] = v;
            maxm = std::max(maxm, npoints[i]);
        }
        std::vector<Fr> d(maxm);
        Fr acc_gamma = Fr::one(), sum = Fr::zero();
        for (size_t i = 0, p = 0; i < k; p += npoints[i], ++i) {
            Fr c = acc_gamma;  // the product over the other sets: z may be a root of Z_(S_i), so no division by zs[i]
            for (size_t l = 0; l < k; ++l)
                if (l != i) c = fp_mul(c, zs[l]);
            coef[i] = c;
            for (size_t j = 0; j < npoints[i]; ++j) d[j] = claimed[p + j];
            newton_from_values(points + p, d.data(), npoints[i]);
            sum = fp_add(sum, fp_mul(c, newton_eval(points + p, d.data(), npoints[i], z)));
            acc_gamma = fp_mul(acc_gamma, gamma);
        }
        Fr zt = Fr::one();
        for (size_t i = 0; i < k; ++i) zt = fp_mul(zt, zs[i]);
        coef[k] = zt;
        coef[k + 1] = sum;
    }
};

}  // namespace gmsm
