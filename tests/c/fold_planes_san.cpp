// Stand-alone host program for the sanitizers (tests/test_fold_planes_sanitized.py builds it as plain C++ under the address
// and undefined-behaviour sanitizers and runs it; no device code, no device, no library): GroupHost::fold_planes of gmsm_group_host.h over fixed
// planes [k]G of BN254 G1 (G = (1, 2)) against the same sum built plane by plane with doublings and additions -
//   sum_w 2^(c w) (k_w0 + sum_(i>=1) 2^(log2L + i - 1) k_wi) [G]
// - at the headline's shape (8 windows of 13 planes), a shape whose windows share bit positions, one window, planes at
// infinity, an empty window and an all-infinite input. Exit status 0: every comparison held.
#include <cstdio>
#include <vector>

#include "gmsm_group_host.h"

using namespace gmsm;

template <class H>
static typename H::Ext times_pow2(typename H::Ext p, unsigned bits) {
    for (unsigned l = 0; l < bits; ++l)
        if (!p.zz.is_zero()) p = xyzz_double(p);
    return p;
}

template <class H>
static bool same_point(const typename H::J &a, const typename H::J &b) {
    using F = typename H::F;
    const Affine<F> x = affine_from_jac(a), y = affine_from_jac(b);
    return memcmp(&x, &y, sizeof x) == 0;
}

// planes[w][i] = [k]G for k from a fixed recurrence; `hole(w, i)` makes a plane infinite
template <class H, class Hole>
static int check(const char *name, const typename H::Aff &gen, unsigned c, unsigned nwin, unsigned log2L, unsigned nhigh, Hole hole) {
    using Ext = typename H::Ext;
    using J = typename H::J;
    const unsigned NP = 7 + nhigh;
    std::vector<Ext> planes((size_t)nwin * NP);
    uint64_t k = 0x9e3779b97f4a7c15ull;
    Ext want = Ext::infinity();
    for (unsigned w = 0; w < nwin; ++w)
        for (unsigned i = 0; i < NP; ++i) {
            k = k * 6364136223846793005ull + 1442695040888963407ull;
            Ext p = hole(w, i) ? Ext::infinity() : H::scalar_mul(gen, &k, 1);
            planes[(size_t)w * NP + i] = p;
            xyzz_add(want, times_pow2<H>(p, c * w + (i == 0 ? 0 : log2L + i - 1)));
        }
    const J got = H::fold_planes(planes.data(), c, nwin, log2L, nhigh);
    const J ref = jac_from_xyzz(want);
    const bool ok = same_point<H>(got, ref) && got.z.is_zero() == ref.z.is_zero();
    printf("%-28s c=%u nwin=%u log2L=%u planes=%u: %s\n", name, c, nwin, log2L, NP, ok ? "ok" : "MISMATCH");
    return ok ? 0 : 1;
}

template <class H>
static int run_group(const char *name, const typename H::Aff &gen) {
    int bad = 0;
    const auto none = [](unsigned, unsigned) { return false; };
    bad += check<H>(name, gen, 16, 8, 3, 6, none);
    bad += check<H>(name, gen, 7, 4, 3, 6, none);  // windows share bit positions
    bad += check<H>(name, gen, 13, 1, 1, 1, none);
    bad += check<H>(name, gen, 11, 3, 4, 0, [](unsigned w, unsigned i) { return w == 1 || (w + i) % 3 == 0 || (w == 2 && i == 6); });
    bad += check<H>(name, gen, 16, 8, 3, 6, [](unsigned, unsigned) { return true; });
    return bad;
}

int main() {
    using Fq = Fp<bn254_fp_params>;
    using H1 = GroupHost<Fq, bn254_fr_params>;
    const H1::Aff g{Fq::one(), fp_dbl(Fq::one())};
    const int bad = run_group<H1>("bn254 g1", g);
    printf("%s\n", bad ? "FAILED" : "all ok");
    return bad ? 1 : 0;
}
