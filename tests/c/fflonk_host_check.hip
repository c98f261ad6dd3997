// Stand-alone host check of FflonkField (gmsm_fflonk.h), no GPU: the divisors, the root of one, the extended sets, both sets
// of claimed values from host-computed chain remainders, the index tables and the refusals, then the same plan in shplonk's
// singleton form, printed for tests/test_fflonk_host.py to compare with tests/fflonk_model.py and tests/shplonk_model.py.
// Built there with AddressSanitizer on the host side.
#include <cstdio>
#include "gmsm_fflonk.h"
using namespace gmsm;
namespace gmsm { int fail(int code, const std::string &msg) { fprintf(stderr, "fail: %s\n", msg.c_str()); return code; } }
template <class FrP> static Fp<FrP> small(unsigned v) { Fp<FrP> a = Fp<FrP>::zero(); for (unsigned i = 0; i < v; ++i) a = fp_add(a, Fp<FrP>::one()); return a; }
template <class FrP> static void put(const char *tag, const Fp<FrP> &x) {
    Fp<FrP> t = fp_from_mont(x);
    printf("%s 0x", tag);
    for (int i = FrP::N - 1; i >= 0; --i) printf("%08x", t.l[i]);
    printf("\n");
}
// the chains' remainders by plain synthetic division on the host
template <class FrP> static std::vector<Fp<FrP>> remainders(const typename FflonkField<FrP>::Plan &p, const std::vector<Fp<FrP>> &flat, const size_t *lens) {
    using Fr = Fp<FrP>;
    std::vector<Fr> rem(p.nrem, Fr::zero());
    size_t off = 0, r = 0;
    for (size_t i = 0, at = 0; i < p.k; at += p.m[i], ++i)
        for (size_t j = 0; j < p.count[i]; off += lens[p.first[i] + j], r += p.m[i], ++j) {
            std::vector<Fr> q(flat.begin() + off, flat.begin() + off + lens[p.first[i] + j]);
            for (size_t c = 0; c < p.m[i] && !q.empty(); ++c) {
                Fr y = Fr::zero();
                std::vector<Fr> ys(q.size());
                for (size_t e = q.size(); e-- > 0;) y = fp_add(q[e], fp_mul(p.a[at + c], y)), ys[e] = y;
                rem[r + c] = ys[0];
                q.assign(ys.begin() + 1, ys.end());
            }
        }
    return rem;
}
template <class FrP> static void put_tables(const char *tag, const typename FflonkField<FrP>::Plan &p, const size_t *lens) {
    std::vector<uint64_t> tbl(p.table_words());
    FflonkField<FrP>::tables(p, lens, tbl.data());
    printf("%s", tag);
    for (uint64_t v : tbl) printf(" %llu", (unsigned long long)v);
    printf("\n");
}
template <class FrP> static void run(const char *name) {
    using FF = FflonkField<FrP>; using Fr = Fp<FrP>;
    printf("field %s\n", name);
    for (size_t n = 1; n <= 16; ++n) { size_t t = 0; FF::next_divisor(n, &t); printf("div %zu %zu\n", n, t); }
    put<FrP>("root6", FF::root_of_one(6));
    // pack 0: 2 polynomials [1,2,3],[4,5] at {3,5}; pack 1: 5 polynomials (t = 6) [7],[],[1,1],[2,0,9,4],[6] at {2}
    std::vector<std::vector<unsigned>> polys = {{1, 2, 3}, {4, 5}, {7}, {}, {1, 1}, {2, 0, 9, 4}, {6}};
    size_t lens[7], pack_sizes[2] = {2, 5}, npoints[2] = {2, 1};
    std::vector<Fr> flat;
    for (size_t j = 0; j < 7; ++j) { lens[j] = polys[j].size(); for (unsigned v : polys[j]) flat.push_back(small<FrP>(v)); }
    Fr pts[3] = {small<FrP>(3), small<FrP>(5), small<FrP>(2)};
    typename FF::Plan p;
    int rc = FF::plan("check", lens, pack_sizes, 2, (const uint64_t *)pts, npoints, true, 1000, &p);
    printf("plan %d maxfold %zu wlen %zu nrem %zu next %zu\n", rc, p.maxfold, p.wlen, p.nrem, p.next);
    for (size_t i = 0; i < p.ext.size(); ++i) put<FrP>("ext", p.ext[i]);
    std::vector<Fr> rem = remainders<FrP>(p, flat, lens);
    std::vector<Fr> claimed(p.next), folded(p.next);
    FF::claimed_values(p, rem.data(), claimed.data(), folded.data());
    for (auto &x : claimed) put<FrP>("claimed", x);
    for (auto &x : folded) put<FrP>("folded", x);
    put_tables<FrP>("tables", p, lens);
    // refusals
    Fr bad[2] = {small<FrP>(1), fp_neg(small<FrP>(1))};
    size_t l2[2] = {3, 3}, ps[1] = {2}, np2[1] = {2};
    printf("equal %d\n", FF::plan("check", l2, ps, 1, (const uint64_t *)bad, np2, true, 1000, &p));
    Fr zero = Fr::zero(); size_t np1[1] = {1};
    printf("zero_t2 %d\n", FF::plan("check", l2, ps, 1, (const uint64_t *)&zero, np1, true, 1000, &p));
    printf("size_short %d\n", FF::plan("check", l2, ps, 1, (const uint64_t *)pts, np2, true, 2 * 3 + 4 - 2, &p));
    printf("size_exact %d\n", FF::plan("check", l2, ps, 1, (const uint64_t *)pts, np2, true, 2 * 3 + 4 - 1, &p));
    // singleton form (pack_sizes == null, shplonk): [1,2,3] at {3,5}, [4,5] at {2}, [7] at {2,9} - a point shared by two sets,
    // and a chain that runs out of coefficients
    size_t slens[3] = {3, 2, 1}, snp[3] = {2, 1, 2};
    std::vector<Fr> sflat(flat.begin(), flat.begin() + 6);
    Fr spts[5] = {small<FrP>(3), small<FrP>(5), small<FrP>(2), small<FrP>(2), small<FrP>(9)};
    rc = FF::plan("check", slens, nullptr, 3, (const uint64_t *)spts, snp, true, 1000, &p);
    printf("s_plan %d maxfold %zu wlen %zu nrem %zu\n", rc, p.maxfold, p.wlen, p.nrem);
    put_tables<FrP>("s_tables", p, slens);
    rem = remainders<FrP>(p, sflat, slens);
    std::vector<Fr> sclaimed(p.np);
    FF::claimed_values(p, rem.data(), sclaimed.data(), nullptr);
    for (auto &x : sclaimed) put<FrP>("s_claimed", x);
    // refusals: a point twice in one set; one point in two sets; a key one base short of max_size + sum m_i - 1, then exact
    Fr twice[2] = {small<FrP>(3), small<FrP>(3)};
    size_t one[1] = {3}, two[1] = {2}, l2s[2] = {3, 3}, np11[2] = {1, 1};
    printf("s_equal %d\n", FF::plan("check", one, nullptr, 1, (const uint64_t *)twice, two, true, 1000, &p));
    printf("s_shared %d\n", FF::plan("check", l2s, nullptr, 2, (const uint64_t *)twice, np11, true, 1000, &p));
    printf("s_size_short %d\n", FF::plan("check", slens, nullptr, 3, (const uint64_t *)spts, snp, true, 3 + 5 - 2, &p));
    printf("s_size_exact %d\n", FF::plan("check", slens, nullptr, 3, (const uint64_t *)spts, snp, true, 3 + 5 - 1, &p));
}
int main() {
    run<bn254_fr_params>("bn254");
    run<bls12_381_fr_params>("bls12_381");
    run<bw6_761_fr_params>("bw6_761");
    return 0;
}
