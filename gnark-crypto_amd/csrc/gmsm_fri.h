// The prover of fr/fri (RADIX_2_FRI, rho = 8, nbRounds = 1) over layers and Merkle trees that never leave HBM: what joins
// fr/fft (gmsm_fft.h), MiMC and the tree over it (gmsm_mimc.h). The Fiat-Shamir transcript stays with the caller, as with a GKR
// claim: an oracle (FriOracle, gmsm_context.h) is committed, then folded once per challenge, then queried.
//
// Replaces, with identical results (every layer element and every node is a uniquely determined element of Fr):
//   FFT(DIF) + BitReverse + sort                 ecc/bn254/fr/fri/fri.go:238-246, :503-506
//   foldPolynomialLagrangeBasis + sort           fri.go:332-355, :404, :426-429
//   the tree of a step, once instead of twice    fri.go:407-411 (the root), :458-466 (the paths)
//   the two proofs of a query                    fri.go:468-485
// and the twins of BLS12-381 and BW6-761. The verifiers are host arithmetic of the size of a proof (fri.py).
//
// Layout. A layer of s elements is kept SORTED, as the reference hashes it: sorted[2i] = e[i], sorted[2i + 1] = e[i + s/2] for the
// evaluations e on the subgroup of order s - the two points of a fibre of x -> x^2 side by side.
//   k_fri_sort_dif   from the DIF transform's output straight to the sorted layer. With m = log2 n: natural[i] = dif[rev_m(i)], and
//                    for i < n/2, rev_m(i) = 2 rev_(m-1)(i) and rev_m(i + n/2) = 2 rev_(m-1)(i) + 1, so
//                    sorted[2i + b] = dif[2 rev_(m-1)(i) + b]: a lane moves one whole pair.
//   k_fri_fold       res[i] = ((p[2i] - p[2i+1]) g^-i x + p[2i] + p[2i+1]) / 2 for i < s/2, written sorted: lane j < s/4 reads the
//                    pairs at 2j and 2j + s/2, computes res[j] and res[j + s/4] and writes them side by side at 2j, 2j + 1. At step
//                    k the generator is w^(2^k) for the domain's w, so g^-j = w^-(j 2^k) and g^-(j + s/4) = w^-(j 2^k + N/4): both
//                    are entries of FftDomain::twiddles_inv_lz (t < N/2), which is in the lazy domain - the factor 2^DOMAIN_SHIFT is
//                    what the lazy product divides by (gmsm_fft_lazy.h), so x and 1/2 come in the same form and every product is the
//                    FFT's own.
//   k_fri_query      one lane per step of a round: the pair of leaves around the queried one, its siblings bottom up with their
//                    count (as k_merkle_prove writes them), and the level-0 sum of the queried leaf, which is the neighbour's
//                    ProofSet[1]: it is in the tree already. Layers and trees are separate allocations: a table of pointers.
// Each kernel is a pure map: no atomics, no flags.
#pragma once
#include <hip/hip_runtime.h>
#include "gmsm_context.h"
#include "gmsm_field.h"
#include "gmsm_fft.h"
#include "gmsm_mimc.h"

namespace gmsm {

constexpr unsigned FRI_TPB = 256;
constexpr unsigned FRI_MIN_LOG2N = 4;  // N >= 16: rho = 8 times a polynomial of size >= 2

template <class FrP>
__global__ void __launch_bounds__(FRI_TPB) k_fri_sort_dif(const Fp<FrP> *__restrict__ dif, size_t half, unsigned log2half,
                                                          Fp<FrP> *__restrict__ sorted) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= half) return;
    const size_t r = fft_bitrev(i, log2half);
    fft_store(sorted, 2 * i, fft_load(dif, 2 * r));
    fft_store(sorted, 2 * i + 1, fft_load(dif, 2 * r + 1));
}

// ((a - b) g x + a + b) / 2 with g, x and 1/2 in the lazy domain
template <class FrP>
__device__ __forceinline__ Fp<FrP> fri_fold_pair(const Fp<FrP> &a, const Fp<FrP> &b, const Fp<FrP> &g_lz, const Fp<FrP> &x_lz,
                                                 const Fp<FrP> &half_lz) {
    using Z = FftLz<FrP>;
    const Fp<FrP> odd = Z::store(Z::mul(Z::mul(Z::load(fp_sub(a, b)), g_lz), x_lz));
    return Z::store(Z::mul(Z::load(fp_add(odd, fp_add(a, b))), half_lz));
}

// in: the sorted layer of 4 quarter elements at step `step`; out: the next one, 2 quarter elements. tw_inv: w^-t, t < N/2 = 2 nq.
template <class FrP>
__global__ void __launch_bounds__(FRI_TPB) k_fri_fold(const Fp<FrP> *__restrict__ in, size_t quarter, unsigned step, size_t nq,
                                                      const Fp<FrP> *__restrict__ tw_inv, const Fp<FrP> x_lz, const Fp<FrP> half_lz,
                                                      Fp<FrP> *__restrict__ out) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= quarter) return;
    const size_t t = j << step;  // < N/4
    const Fp<FrP> lo = fri_fold_pair(fft_load(in, 2 * j), fft_load(in, 2 * j + 1), fft_load(tw_inv, t), x_lz, half_lz);
    const size_t u = 2 * (j + quarter);
    const Fp<FrP> hi = fri_fold_pair(fft_load(in, u), fft_load(in, u + 1), fft_load(tw_inv, t + nq), x_lz, half_lz);
    fft_store(out, 2 * j, lo);
    fft_store(out, 2 * j + 1, hi);
}

template <class Fr>
struct FriQueryStep {
    const Fr *layer;  // n sorted evaluations
    const Fr *nodes;  // the levels of the tree over them
    unsigned long long n, pos;  // pos < n, n even
};

// Step j < count: out_pairs[2j, 2j + 1] = the leaves at pos & ~1 and next to it, out_leaf_sums[j] = H(leaf pos), the siblings of
// leaf pos bottom up into out_siblings[j stride ..] with zeros behind them (stride >= the depth of every tree), their number
// into out_counts[j].
template <class FrP>
__global__ void __launch_bounds__(FRI_TPB) k_fri_query(const FriQueryStep<Fp<FrP>> *__restrict__ steps, size_t count, unsigned stride,
                                                       Fp<FrP> *__restrict__ out_pairs, Fp<FrP> *__restrict__ out_leaf_sums,
                                                       Fp<FrP> *__restrict__ out_siblings, uint32_t *__restrict__ out_counts) {
    using Fr = Fp<FrP>;
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count) return;
    const FriQueryStep<Fr> st = steps[j];
    size_t idx = (size_t)st.pos, size = (size_t)st.n;
    const size_t even = idx & ~(size_t)1;
    fft_store(out_pairs, 2 * j, fft_load(st.layer, even));
    fft_store(out_pairs, 2 * j + 1, fft_load(st.layer, even + 1));
    fft_store(out_leaf_sums, j, fft_load(st.nodes, idx));
    const Fr *level = st.nodes;
    uint32_t cnt = 0;
    for (; size > 1; level += size, size = (size + 1) / 2, idx >>= 1) {
        const size_t sib = idx ^ 1;
        if (sib < size) fft_store(out_siblings, j * stride + cnt++, fft_load(level, sib));
    }
    for (uint32_t l = cnt; l < stride; ++l) fft_store(out_siblings, j * stride + l, Fr::zero());
    out_counts[j] = cnt;
}

// ------------------------------------------------------------------ host side of one scalar field
template <class FrP>
struct FriField {
    using Fr = Fp<FrP>;
    using MF = MimcField<FrP>;

    // a tree of n leaves of one element with its buffers: `leaves` is the layer the fold (or the sort) writes
    static int new_tree(const FriOracle &o, size_t n, std::unique_ptr<MerkleTree> *out) {
        std::unique_ptr<MerkleTree> t(new MerkleTree());
        t->group = o.group, t->device = o.device, t->n = n, t->leaf_len = 1;
        for (size_t size = n;; size = (size + 1) / 2) {
            t->total += size;
            if (size == 1) break;
            ++t->depth;
        }
        int rc;
        if ((rc = t->leaves.ensure(n * sizeof(Fr))) || (rc = t->nodes.ensure(t->total * sizeof(Fr)))) return rc;
        *out = std::move(t);
        return GMSM_OK;
    }

    static int commit(Context &ctx, FriOracle *oracle, const uint64_t *p, const void *d_p, size_t len, hipStream_t caller) {
        const char *E = "gmsm_fri_commit";
        FriOracle &o = *oracle;
        GMSM_LEASE_OR_FAIL(lease, ctx);
        Workspace &ws = *lease.w;
        const size_t N = (size_t)1 << o.log2n;
        int rc;
        std::unique_ptr<MerkleTree> t;
        if ((rc = ws.h2d_scalars.ensure(N * sizeof(Fr))) || (rc = new_tree(o, N, &t))) return rc;
        Fr *v = (Fr *)ws.h2d_scalars.ptr;  // the transform's vector: p is never modified
        DrainOnExit drain{ws.stream};
        if (d_p && (rc = order_after(ws, caller))) return rc;
        if (len) HIP_TRY(hipMemcpyAsync(v, p ? (const void *)p : d_p, len * sizeof(Fr), p ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, ws.stream));
        if (len < N) HIP_TRY(hipMemsetAsync(v + len, 0, (N - len) * sizeof(Fr), ws.stream));
        {
            std::lock_guard<std::mutex> lk(o.domain->mu);
            rc = FftField<FrP>::run(ws.stream, o.domain.get(), v, false, true, false);
        }
        if (rc) return rc;
        hipLaunchKernelGGL((k_fri_sort_dif<FrP>), dim3((unsigned)((N / 2 + FRI_TPB - 1) / FRI_TPB)), dim3(FRI_TPB), 0, ws.stream, (const Fr *)v, N / 2,
                           o.log2n - 1, (Fr *)t->leaves.ptr);
        HIP_TRY(hipGetLastError());
        if ((rc = MF::merkle_build(E, ws.stream, *t, (const Fr *)t->leaves.ptr))) return rc;
        HIP_TRY(hipStreamSynchronize(ws.stream));
        o.trees.push_back(std::move(t));
        return GMSM_OK;
    }

    static Fr lazy(const Fr &x) { return fp_mul(x, FftField<FrP>::lazy_shift()); }

    // folds_done < nb_steps. out: the new layer's root, or the Evaluation after the last fold
    static int fold(Context &ctx, FriOracle *oracle, const uint64_t *xi, uint64_t *out) {
        const char *E = "gmsm_fri_fold";
        FriOracle &o = *oracle;
        GMSM_LEASE_OR_FAIL(lease, ctx);
        Workspace &ws = *lease.w;
        const unsigned k = o.folds_done;
        const size_t N = (size_t)1 << o.log2n, quarter = (N >> k) / 4;
        const bool last = k + 1 == o.nb_steps;
        int rc;
        std::unique_ptr<MerkleTree> t;
        if ((rc = last ? o.last.ensure(2 * quarter * sizeof(Fr)) : new_tree(o, 2 * quarter, &t))) return rc;
        Fr *next = last ? (Fr *)o.last.ptr : (Fr *)t->leaves.ptr;
        const Fr x_lz = lazy(fr_from_limbs<Fr>(xi)), half_lz = lazy(fp_inv(fp_dbl(Fr::one())));
        DrainOnExit drain{ws.stream};
        hipLaunchKernelGGL((k_fri_fold<FrP>), dim3((unsigned)((quarter + FRI_TPB - 1) / FRI_TPB)), dim3(FRI_TPB), 0, ws.stream,
                           (const Fr *)o.trees[k]->leaves.ptr, quarter, k, N / 4, (const Fr *)o.domain->twiddles_inv_lz.ptr, x_lz, half_lz, next);
        HIP_TRY(hipGetLastError());
        if (last) {
            o.evaluation.resize(sizeof(Fr) / 8);
            HIP_TRY(hipMemcpyAsync(o.evaluation.data(), next, sizeof(Fr), hipMemcpyDeviceToHost, ws.stream));
        } else if ((rc = MF::merkle_build(E, ws.stream, *t, (const Fr *)next))) {
            return rc;
        }
        HIP_TRY(hipStreamSynchronize(ws.stream));
        if (!last) o.trees.push_back(std::move(t));
        ++o.folds_done;
        memcpy(out, last ? o.evaluation.data() : o.trees.back()->root.data(), sizeof(Fr));
        return GMSM_OK;
    }

    static int layer(Context &ctx, FriOracle *oracle, unsigned step, uint64_t *out, void *d_out) {
        FriOracle &o = *oracle;
        GMSM_LEASE_OR_FAIL(lease, ctx);
        Workspace &ws = *lease.w;
        const size_t bytes = (((size_t)1 << o.log2n) >> step) * sizeof(Fr);
        if (d_out) HIP_TRY(hipDeviceSynchronize());  // the entry takes no stream: d_out may still be in use on one we do not know
        HIP_TRY(hipMemcpyAsync(out ? (void *)out : d_out, o.trees[step]->leaves.ptr, bytes, out ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice,
                               ws.stream));
        HIP_TRY(hipStreamSynchronize(ws.stream));
        return GMSM_OK;
    }

    // 0 < count <= the layers built, positions[i] below layer i's size. The outputs of step i: out_pairs[2i ..], out_leaf_sums[i],
    // out_siblings[i log2n ..], out_counts[i].
    static int query(Context &ctx, FriOracle *oracle, const uint64_t *positions, size_t count, uint64_t *out_pairs, uint64_t *out_leaf_sums,
                     uint64_t *out_siblings, uint32_t *out_counts) {
        FriOracle &o = *oracle;
        GMSM_LEASE_OR_FAIL(lease, ctx);
        Workspace &ws = *lease.w;
        const unsigned stride = o.log2n;
        const size_t pair_bytes = 2 * count * sizeof(Fr), sum_bytes = count * sizeof(Fr), sib_bytes = count * stride * sizeof(Fr);
        const size_t sum_at = pair_bytes, sib_at = sum_at + sum_bytes, cnt_at = sib_at + sib_bytes;
        const size_t tab_at = (cnt_at + count * sizeof(uint32_t) + 15) & ~(size_t)15;
        int rc = ws.poly.ensure(tab_at + count * sizeof(FriQueryStep<Fr>));
        if (rc) return rc;
        unsigned char *buf = (unsigned char *)ws.poly.ptr;
        std::vector<FriQueryStep<Fr>> tab(count);
        for (size_t i = 0; i < count; ++i)
            tab[i] = FriQueryStep<Fr>{(const Fr *)o.trees[i]->leaves.ptr, (const Fr *)o.trees[i]->nodes.ptr, o.trees[i]->n, positions[i]};
        DrainOnExit drain{ws.stream};
        HIP_TRY(hipMemcpyAsync(buf + tab_at, tab.data(), count * sizeof(FriQueryStep<Fr>), hipMemcpyHostToDevice, ws.stream));
        hipLaunchKernelGGL((k_fri_query<FrP>), dim3((unsigned)((count + FRI_TPB - 1) / FRI_TPB)), dim3(FRI_TPB), 0, ws.stream,
                           (const FriQueryStep<Fr> *)(buf + tab_at), count, stride, (Fr *)buf, (Fr *)(buf + sum_at), (Fr *)(buf + sib_at),
                           (uint32_t *)(buf + cnt_at));
        HIP_TRY(hipGetLastError());
        // one copy back, scattered to the caller's four arrays on the host
        std::vector<unsigned char> host(cnt_at + count * sizeof(uint32_t));
        HIP_TRY(hipMemcpyAsync(host.data(), buf, host.size(), hipMemcpyDeviceToHost, ws.stream));
        HIP_TRY(hipStreamSynchronize(ws.stream));
        memcpy(out_pairs, host.data(), pair_bytes);
        memcpy(out_leaf_sums, host.data() + sum_at, sum_bytes);
        memcpy(out_siblings, host.data() + sib_at, sib_bytes);
        memcpy(out_counts, host.data() + cnt_at, count * sizeof(uint32_t));
        return GMSM_OK;
    }
};

}  // namespace gmsm
