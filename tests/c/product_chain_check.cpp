// Host-side check of the Montgomery product scans of gmsm_fieldu.h - fpu_mul, fpu_mul_add, fpu_mul_add4, fpu_sqr and the
// two-at-once forms fpu_mul2 / fpu_sqr2, on unsigned and on signed limbs - against big-integer arithmetic, for the three
// base fields in scope (9 x 29, 14 x 28 and 28 x 28 bit limbs). A scan of the products a_j b_j returns r with
//     r * 2^(L W) = sum_j a_j b_j + M q,   0 <= M < 2^(L W)
// as an identity of integers (M = the Montgomery digits), so the check is exact and needs no second field implementation:
//     D = r * 2^(L W) - sum_j a_j b_j   satisfies   0 <= D < 2^(L W) q   and   D = 0 mod q,
// which is both the residue a b 2^-(L W) mod q and the documented range (sum/R <= r < sum/R + q: for |sum| < A R the result
// lies in (-A, A + q)); the low limbs of r must be normalised, [0, 2^W), and the top limb carries the rest (and the sign).
// Operands: every limb at the admitted extreme +-(2^W + 2^(32-W)) (all one sign, and alternating) with the top limb at
// the bound the call sites state (values below 18 q for the unsigned additions, within +-8 q on signed limbs); the values
// 0, 1, q - 1, q, 2q - 1; and 10 000 random pairs per field with limbs anywhere in the admitted range. fpu_mul_add4 is
// compiled only where its column accumulators hold 5L products (BLS12-381; its static_assert says so for the others).
// The program is meant for -fsanitize=undefined,address: a signed column that overflows is undefined behaviour there.
// Exit code = number of mismatches (capped).
// Build: clang++ -O1 -std=c++17 -D__host__= -D__device__= -D__noinline__= -D__forceinline__=inline tests/c/product_chain_check.cpp
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../gnark-crypto_amd/csrc/gmsm_params32.h"
#include "../../gnark-crypto_amd/csrc/gmsm_fieldu.h"
using namespace gmsm;

// ---- fixed-width two's complement integers: 28 x 64 = 1792 bits (operands < 2^790, sums of four products < 2^1582)
static constexpr int NW = 28, HW = 14;
struct Big {
    uint64_t w[NW];
};
static Big big_zero() {
    Big z;
    memset(&z, 0, sizeof z);
    return z;
}
static bool big_neg(const Big &a) { return (a.w[NW - 1] >> 63) != 0; }
static Big big_add(const Big &a, const Big &b) {
    Big r;
    unsigned __int128 c = 0;
    for (int i = 0; i < NW; ++i) {
        c += (unsigned __int128)a.w[i] + b.w[i];
        r.w[i] = (uint64_t)c;
        c >>= 64;
    }
    return r;
}
static Big big_negate(const Big &a) {
    Big r;
    unsigned __int128 c = 1;
    for (int i = 0; i < NW; ++i) {
        c += (uint64_t)~a.w[i];
        r.w[i] = (uint64_t)c;
        c >>= 64;
    }
    return r;
}
static Big big_sub(const Big &a, const Big &b) { return big_add(a, big_negate(b)); }
static bool big_is_zero(const Big &a) {
    uint64_t o = 0;
    for (int i = 0; i < NW; ++i) o |= a.w[i];
    return o == 0;
}
static bool big_less(const Big &a, const Big &b) { return big_neg(big_sub(a, b)); }  // no overflow at these sizes
// x += v * 2^bit for a magnitude v < 2^33
static void big_add_shifted(Big &x, uint64_t v, int bit) {
    const int word = bit >> 6, sh = bit & 63;
    unsigned __int128 c = (unsigned __int128)v << sh;
    for (int i = word; i < NW && c != 0; ++i) {
        c += x.w[i];
        x.w[i] = (uint64_t)c;
        c >>= 64;
    }
}
static Big big_shl(const Big &a, int bits) {
    Big r = big_zero();
    const int word = bits >> 6, sh = bits & 63;
    for (int i = NW - 1; i >= word; --i) {
        uint64_t v = a.w[i - word] << sh;
        if (sh && i - word - 1 >= 0) v |= a.w[i - word - 1] >> (64 - sh);
        r.w[i] = v;
    }
    return r;
}
// signed product of two values below 2^(64 HW - 1) in magnitude
static Big big_mul(const Big &a, const Big &b) {
    const bool na = big_neg(a), nb = big_neg(b);
    const Big x = na ? big_negate(a) : a, y = nb ? big_negate(b) : b;
    Big r = big_zero();
    for (int i = 0; i < HW; ++i) {
        unsigned __int128 c = 0;
        for (int j = 0; j < HW; ++j) {
            c += (unsigned __int128)x.w[i] * y.w[j] + r.w[i + j];
            r.w[i + j] = (uint64_t)c;
            c >>= 64;
        }
        // (i + HW <= NW - 1 for every i < HW)
        r.w[i + HW] += (uint64_t)c;
    }
    return na != nb ? big_negate(r) : r;
}

// ---- per field: q, 2^(L W) q, and 2^(64 j) mod q for the divisibility test
template <class P>
struct Ref {
    static constexpr int L = P::UL, W = P::UW;
    static constexpr int QW = (P::N + 1) / 2;  // 64-bit words of q
    Big q, rq;
    Big pow64[NW];    // 2^(64 j) mod q
    Big qshift[72];   // q * 2^s
    Ref() {
        q = big_zero();
        for (int i = 0; i < P::N; ++i) big_add_shifted(q, P::Q[i], 32 * i);
        rq = big_shl(q, L * W);
        for (int s = 0; s < 72; ++s) qshift[s] = big_shl(q, s);
        Big t = big_zero();
        t.w[0] = 1;
        for (int j = 0; j < NW; ++j) {
            pow64[j] = t;
            for (int k = 0; k < 64; ++k) {
                t = big_add(t, t);
                if (!big_less(t, q)) t = big_sub(t, q);
            }
        }
    }
    // x = 0 mod q, for 0 <= x
    bool divisible(const Big &x) const {
        Big acc = big_zero();
        for (int j = 0; j < QW; ++j) acc.w[j] = x.w[j];
        for (int j = QW; j < NW; ++j) {
            if (x.w[j] == 0) continue;
            unsigned __int128 c = 0;  // acc += x.w[j] * pow64[j]
            for (int i = 0; i < NW; ++i) {
                c += (unsigned __int128)x.w[j] * (i < QW ? pow64[j].w[i] : 0u) + acc.w[i];
                acc.w[i] = (uint64_t)c;
                c >>= 64;
            }
        }
        // acc < 2^(64 QW) + NW 2^64 q < 2^72 q for the three fields
        for (int s = 71; s >= 0; --s)
            if (!big_less(acc, qshift[s])) acc = big_sub(acc, qshift[s]);
        return big_is_zero(acc);
    }
};

template <class P, bool SIGNED>
static Big value_of(const FpU<P> &a) {
    Big pos = big_zero(), neg = big_zero();
    for (int i = 0; i < P::UL; ++i) {
        const int64_t v = SIGNED ? (int64_t)(int32_t)a.l[i] : (int64_t)a.l[i];
        if (v >= 0) big_add_shifted(pos, (uint64_t)v, P::UW * i);
        else big_add_shifted(neg, (uint64_t)(-v), P::UW * i);
    }
    return big_sub(pos, neg);
}

template <class P, bool SIGNED>
struct Checker {
    using U = FpU<P>;
    const Ref<P> &ref;
    const char *field;
    long checks = 0;
    int bad = 0;
    Checker(const Ref<P> &r, const char *f) : ref(r), field(f) {}

    // r against the products ops[0] ops[1] + ops[2] ops[3] + ...
    void expect(const char *what, const U &r, std::initializer_list<const U *> ops) {
        Big sum = big_zero();
        for (auto it = ops.begin(); it != ops.end(); it += 2) sum = big_add(sum, big_mul(value_of<P, SIGNED>(**it), value_of<P, SIGNED>(**(it + 1))));
        const Big d = big_sub(big_shl(value_of<P, SIGNED>(r), P::UL * P::UW), sum);
        bool ok = !big_neg(d) && big_less(d, ref.rq) && ref.divisible(d);
        for (int i = 0; i < P::UL - 1; ++i) ok = ok && (r.l[i] >> P::UW) == 0;
        ++checks;
        if (!ok && bad++ < 5) printf("%s %s %s: wrong result at check %ld\n", field, SIGNED ? "signed" : "unsigned", what, checks);
    }

    void products(const U &a, const U &b, const U &c, const U &d) {
        expect("fpu_mul", fpu_mul<P, SIGNED>(a, b), {&a, &b});
        expect("fpu_sqr", fpu_sqr<P, SIGNED>(a), {&a, &a});
        expect("fpu_mul_add", fpu_mul_add<P, SIGNED>(a, b, c, d), {&a, &b, &c, &d});
#ifdef GMSM_PRODUCT_PAIRS_MAXL  // the header has the two-at-once forms
        const FpuPair<P> m = fpu_mul2<P, SIGNED>(a, b, c, d);
        expect("fpu_mul2.0", m.r0, {&a, &b});
        expect("fpu_mul2.1", m.r1, {&c, &d});
        const FpuPair<P> s = fpu_sqr2<P, SIGNED>(b, d);
        expect("fpu_sqr2.0", s.r0, {&b, &b});
        expect("fpu_sqr2.1", s.r1, {&d, &d});
#endif
        if constexpr (FpsFits4<P>::value) expect("fpu_mul_add4", fpu_mul_add4<P, SIGNED>(a, b, c, d, b, c, d, a), {&a, &b, &c, &d, &b, &c, &d, &a});
    }
};

// the top limb of a value just below K q whose low limbs all sit at the extreme
template <class P>
static uint32_t top_below(unsigned K) { return K * P::UQ1[P::UL - 1] - 2u; }

template <class P, bool SIGNED>
static std::vector<FpU<P>> edge_operands() {
    constexpr int L = P::UL, W = P::UW;
    const uint32_t E = (1u << W) + (1u << (32 - W));
    const uint32_t T = top_below<P>(SIGNED ? 8 : 18);
    std::vector<FpU<P>> v;
    FpU<P> x;
    for (int kind = 0; kind < 5; ++kind) {  // 0, 1, q - 1, q, 2q - 1
        for (int i = 0; i < L; ++i) x.l[i] = kind == 0 ? 0u : kind == 1 ? (i == 0 ? 1u : 0u) : kind == 4 ? P::UQ2[i] : P::UQ1[i];
        if (kind == 2 || kind == 4) x.l[0] -= 1;  // q is odd and the first limb of 2q is not zero: no borrow
        v.push_back(x);
    }
    for (int i = 0; i < L; ++i) x.l[i] = i < L - 1 ? E : T;  // every limb at the upper extreme
    v.push_back(x);
    if (SIGNED) {
        for (int i = 0; i < L; ++i) x.l[i] = 0u - (i < L - 1 ? E : T);  // the lower extreme
        v.push_back(x);
        for (int i = 0; i < L; ++i) x.l[i] = (i & 1) ? 0u - (i < L - 1 ? E : T) : (i < L - 1 ? E : T);  // alternating
        v.push_back(x);
        for (int i = 0; i < L; ++i) x.l[i] = (i & 1) ? (i < L - 1 ? E : T) : 0u - (i < L - 1 ? E : T);
        v.push_back(x);
    }
    return v;
}

template <class P, bool SIGNED>
static FpU<P> random_operand(std::mt19937_64 &g) {
    constexpr int L = P::UL, W = P::UW;
    const uint64_t E = (1ull << W) + (1ull << (32 - W));
    const uint64_t T = top_below<P>(SIGNED ? 8 : 18);
    const bool any_sign = SIGNED && (g() & 1);
    FpU<P> x;
    for (int i = 0; i < L; ++i) {
        const uint64_t lim = i < L - 1 ? E : T;
        const uint32_t mag = (uint32_t)(g() % (lim + 1));
        x.l[i] = any_sign && (g() & 1) ? 0u - mag : mag;
    }
    return x;
}

template <class P, bool SIGNED>
static int run(const Ref<P> &ref, const char *field) {
    Checker<P, SIGNED> ck(ref, field);
    const std::vector<FpU<P>> e = edge_operands<P, SIGNED>();
    const size_t n = e.size();
    for (size_t i = 0; i < n; ++i)
        for (size_t j = 0; j < n; ++j) {
            ck.products(e[i], e[j], e[(i + 1) % n], e[(j + 3) % n]);
            ck.products(e[i], e[j], e[i], e[j]);  // both products of a column at the same extreme
        }
    std::mt19937_64 g(0x9c0 + P::UL + (SIGNED ? 1 : 0));
    FpU<P> c = random_operand<P, SIGNED>(g), d = random_operand<P, SIGNED>(g);
    for (int t = 0; t < 10000; ++t) {
        const FpU<P> a = random_operand<P, SIGNED>(g), b = random_operand<P, SIGNED>(g);
        ck.products(a, b, c, d);  // the second product of the merged scans: the previous pair
        c = a;
        d = b;
    }
    printf("%s %s: %ld checks, %d mismatches\n", field, SIGNED ? "signed" : "unsigned", ck.checks, ck.bad);
    return ck.bad;
}

template <class P>
static int run_field(const char *field) {
    static const Ref<P> ref;
    return run<P, false>(ref, field) + run<P, true>(ref, field);
}

int main() {
    int bad = run_field<bn254_fp_params>("bn254 fp");
    bad += run_field<bls12_381_fp_params>("bls12-381 fp");
    bad += run_field<bw6_761_fp_params>("bw6-761 fp");
    return bad > 100 ? 100 : bad;
}
