// MiMC over a curve's scalar field, in batches, and Merkle trees over it: the hash the reference's proving stacks are built
// around (fr/mimc is what gnark proves in-circuit; accumulator/merkletree over it is what fr/fri commits every round with).
//
// Replaces, with identical results (every digest is a uniquely determined element of Fr, stored canonically in Montgomery form):
//   (*digest).checksum / encrypt            ecc/bn254/fr/mimc/mimc.go:130-163 (Miyaguchi-Preneel: h <- E_h(m) + h + m, E_h(m) =
//                                           the round t <- (t + h + c_i)^5 applied MIMC_ROUNDS times, plus h)
//   GetConstants                            mimc.go:47-54 (the table itself: tools/gen_params.py, FrP::MIMC_C)
//   (*Tree).Push / Root / Prove             accumulator/merkletree/tree.go:137-365, with leafSum(data) = H(data) and
//                                           nodeSum(a, b) = H(a || b) (the prefixes are commented out there, tree.go:92-105)
// and the twins of BLS12-381 (111 rounds) and BW6-761 (163 rounds).
//
// The tree's shape. The reference keeps a stack of complete subtrees and joins the smaller ones first (RFC 6962). The same
// tree, level by level: pair up the nodes of a level from the left; an odd last node has no sibling and moves up unchanged
// until it has one. tests/mimc_model.py restates the reference's algorithm and checks both forms against each other, roots
// and proof sets, for every index of every n up to 40. A proof set lists a node's sibling at every level where it has one,
// bottom up, so paths of one tree may differ in length: a level where the node is the odd last one adds nothing.
//
// Shape on the GPU. One hash is a chain of 3 MIMC_ROUNDS dependent products per element; many hashes are independent, so:
//   k_mimc_batch     one lane per message, h and t in registers, the round constant read at a wave-uniform address; message
//                    i is the `len` elements at i * stride. The loads are strided over the lanes: one 32-byte element buys
//                    330 products. The leaves of a tree are one such batch (leaf i = leaf_len elements at i * leaf_len).
//   k_merkle_level   one lane per parent: two blocks over its children, or the copy of the odd last node.
//   k_merkle_top     every level from MERKLE_TOP nodes down to the root in ONE workgroup, a barrier between levels: the top of
//                    the tree is a chain of log2 small steps that would otherwise each cost a launch.
//   k_merkle_prove   one lane per path: the siblings bottom up, their count, and the leaf's data when it was kept.
// The levels lie one after another in one allocation (level 0 = the leaves' sums, then ceil(n / 2) nodes, ... , the root).
// No atomics, no flags: the hand-off between levels is the kernel boundary or the workgroup barrier.
#pragma once
#include <hip/hip_runtime.h>
#include "gmsm_context.h"
#include "gmsm_field.h"
#include "gmsm_fft.h"

namespace gmsm {

constexpr unsigned MIMC_TPB = 256;
constexpr size_t MERKLE_TOP = 2 * MIMC_TPB;  // k_merkle_top takes a level of at most this many nodes: one lane per parent

template <class FrP>
GMSM_HD Fp<FrP> mimc_constant(unsigned i) {
    Fp<FrP> c;
#pragma unroll
    for (int k = 0; k < FrP::N; ++k) c.l[k] = FrP::MIMC_C[i * FrP::N + k];
    return c;
}

// one block: h <- E_h(m) + h + m. The products are inlined: through the call ABI the second operand of a 12-limb product
// would travel through scratch memory (gmsm_field.h).
template <class FrP>
__device__ __forceinline__ Fp<FrP> mimc_block(const Fp<FrP> &h, const Fp<FrP> &m) {
    using Fr = Fp<FrP>;
    Fr t = m;
#pragma nounroll
    for (unsigned i = 0; i < FrP::MIMC_ROUNDS; ++i) {
        const Fr x = fp_add(fp_add(t, h), mimc_constant<FrP>(i));  // uniform: scalar loads
        const Fr x2 = fp_mul_inline(x, x);
        t = fp_mul_inline(fp_mul_inline(x2, x2), x);
    }
    return fp_add(fp_add(fp_add(t, h), h), m);
}

// the same on the host, for the hash under a Fiat-Shamir transcript (gmsm_mimc_hash): a few blocks, never worth a launch
template <class FrP>
static inline Fp<FrP> mimc_block_host(const Fp<FrP> &h, const Fp<FrP> &m) {
    using Fr = Fp<FrP>;
    Fr t = m;
    for (unsigned i = 0; i < FrP::MIMC_ROUNDS; ++i) {
        const Fr x = fp_add(fp_add(t, h), mimc_constant<FrP>(i));
        const Fr x2 = fp_sqr(x);
        t = fp_mul(fp_sqr(x2), x);
    }
    return fp_add(fp_add(fp_add(t, h), h), m);
}

// out[i] = MiMC from `state` over msgs[i stride .. i stride + len), i < count
template <class FrP>
__global__ void __launch_bounds__(MIMC_TPB) k_mimc_batch(const Fp<FrP> *__restrict__ msgs, size_t count, size_t len, size_t stride,
                                                         const Fp<FrP> state, Fp<FrP> *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    Fp<FrP> h = state;
#pragma nounroll
    for (size_t j = 0; j < len; ++j) h = mimc_block(h, fft_load(msgs, i * stride + j));
    fft_store(out, i, h);
}

// parent p < ceil(n_in / 2) of one level: H(in[2p] || in[2p + 1]), or in[2p] itself when it is the odd last node
template <class FrP>
__device__ __forceinline__ void merkle_parent(const Fp<FrP> *in, size_t n_in, size_t p, Fp<FrP> *out) {
    using Fr = Fp<FrP>;
    Fr h = fft_load(in, 2 * p);
    if (2 * p + 1 < n_in) h = mimc_block(mimc_block(Fr::zero(), h), fft_load(in, 2 * p + 1));
    fft_store(out, p, h);
}

template <class FrP>
__global__ void __launch_bounds__(MIMC_TPB) k_merkle_level(const Fp<FrP> *__restrict__ in, size_t n_in, Fp<FrP> *__restrict__ out) {
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < (n_in + 1) / 2) merkle_parent(in, n_in, p, out);
}

// One workgroup of MIMC_TPB lanes: from the level of n_in <= MERKLE_TOP nodes at `level` up to the root; each level is written
// right behind the one it is made from. n_in is uniform, so every lane reaches every barrier.
template <class FrP>
__global__ void __launch_bounds__(MIMC_TPB) k_merkle_top(Fp<FrP> *level, size_t n_in) {
    while (n_in > 1) {
        const size_t parents = (n_in + 1) / 2;
        if (threadIdx.x < parents) merkle_parent(level, n_in, threadIdx.x, level + n_in);
        __syncthreads();  // the next level reads what other lanes of this workgroup wrote
        level += n_in, n_in = parents;
    }
}

// Path j < k of the tree over n leaves (`nodes`: its levels, `depth` of them above the leaves): the siblings of leaf
// indices[j] bottom up into out_siblings[j depth ..], zeros behind them, their number into out_counts[j]; with `leaves`, the
// leaf's leaf_len elements into out_leaves[j leaf_len ..]. Every index is < n (the entry has checked them).
template <class FrP>
__global__ void __launch_bounds__(MIMC_TPB) k_merkle_prove(const Fp<FrP> *__restrict__ nodes, size_t n, unsigned depth,
                                                           const Fp<FrP> *__restrict__ leaves, size_t leaf_len,
                                                           const unsigned long long *__restrict__ indices, size_t k,
                                                           Fp<FrP> *__restrict__ out_siblings, uint32_t *__restrict__ out_counts,
                                                           Fp<FrP> *__restrict__ out_leaves) {
    using Fr = Fp<FrP>;
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= k) return;
    size_t idx = (size_t)indices[j], size = n;
    if (leaves)
        for (size_t e = 0; e < leaf_len; ++e) fft_store(out_leaves, j * leaf_len + e, fft_load(leaves, idx * leaf_len + e));
    const Fr *level = nodes;
    uint32_t cnt = 0;
    for (unsigned l = 0; l < depth; ++l) {
        const size_t sib = idx ^ 1;
        if (sib < size) fft_store(out_siblings, j * depth + cnt++, fft_load(level, sib));
        level += size, size = (size + 1) / 2, idx >>= 1;
    }
    for (uint32_t l = cnt; l < depth; ++l) fft_store(out_siblings, j * depth + l, Fr::zero());
    out_counts[j] = cnt;
}

// ------------------------------------------------------------------ host side of one scalar field
template <class FrP>
struct MimcField {
    using Fr = Fp<FrP>;

    static void constants(uint64_t *out) {
        for (unsigned i = 0; i < FrP::MIMC_ROUNDS; ++i) {
            const Fr c = mimc_constant<FrP>(i);
            memcpy(out + i * (sizeof(Fr) / 8), &c, sizeof c);
        }
    }
    static void hash(const uint64_t *state, const uint64_t *elems, size_t len, uint64_t *out) {
        Fr h = state ? fr_from_limbs<Fr>(state) : Fr::zero();
        for (size_t j = 0; j < len; ++j) h = mimc_block_host(h, fr_from_limbs<Fr>(elems + j * (sizeof(Fr) / 8)));
        memcpy(out, &h, sizeof h);
    }

    static int grid(const char *E, size_t lanes, unsigned *blocks) {
        const size_t b = (lanes + MIMC_TPB - 1) / MIMC_TPB;
        if (b > 0x7fffffffu) return fail(GMSM_ERR_ARG, std::string(E) + ": too many hashes for one launch");
        *blocks = (unsigned)b;
        return GMSM_OK;
    }
    static int batch_launch(const char *E, hipStream_t s, const Fr *msgs, size_t count, size_t len, size_t stride, const Fr &state, Fr *out) {
        unsigned blocks;
        if (int rc = grid(E, count, &blocks)) return rc;
        hipLaunchKernelGGL((k_mimc_batch<FrP>), dim3(blocks), dim3(MIMC_TPB), 0, s, msgs, count, len, stride, state, out);
        HIP_TRY(hipGetLastError());
        return GMSM_OK;
    }

    // the extent of a batch's input in elements (count > 0)
    static size_t batch_extent(size_t count, size_t len, size_t stride) { return len ? (count - 1) * stride + len : 0; }

    static int sum_batch(Context &ctx, const uint64_t *msgs, const void *d_msgs, size_t count, size_t len, size_t stride, const uint64_t *state,
                         hipStream_t caller, uint64_t *out, void *d_out) {
        const char *E = "gmsm_mimc_sum_batch";
        GMSM_LEASE_OR_FAIL(lease, ctx);
        Workspace &ws = *lease.w;
        const void *in;
        DrainOnExit drain{ws.stream};
        int rc = stage_input(ws, ws.h2d_scalars, msgs, d_msgs, batch_extent(count, len, stride) * sizeof(Fr), {After::STREAM, caller}, &in);
        if (rc) return rc;
        if (d_out && (msgs || !len) && (rc = order_after(ws, caller))) return rc;  // the caller's stream may still use d_out
        if (out && (rc = ws.poly.ensure(count * sizeof(Fr)))) return rc;
        Fr *res = out ? (Fr *)ws.poly.ptr : (Fr *)d_out;
        if ((rc = batch_launch(E, ws.stream, (const Fr *)in, count, len, stride, state ? fr_from_limbs<Fr>(state) : Fr::zero(), res))) return rc;
        if (out) HIP_TRY(hipMemcpyAsync(out, res, count * sizeof(Fr), hipMemcpyDeviceToHost, ws.stream));
        HIP_TRY(hipStreamSynchronize(ws.stream));
        return GMSM_OK;
    }

    // ---- one tree (MerkleTree, gmsm_context.h). The engine has set its shape (group, device, n, leaf_len, depth, total).
    static int merkle_new(Context &ctx, MerkleTree *tree, const uint64_t *leaves, const void *d_leaves, bool keep, hipStream_t caller) {
        const char *E = "gmsm_merkle_new";
        MerkleTree &t = *tree;
        GMSM_LEASE_OR_FAIL(lease, ctx);
        Workspace &ws = *lease.w;
        const size_t leaf_bytes = t.n * t.leaf_len * sizeof(Fr);
        int rc;
        if ((rc = t.nodes.ensure(t.total * sizeof(Fr))) || (keep && (rc = t.leaves.ensure(leaf_bytes)))) return rc;
        DrainOnExit drain{ws.stream};
        const void *in;
        if (keep) {  // the tree's own copy, which the proofs read
            if (d_leaves && (rc = order_after(ws, caller))) return rc;
            HIP_TRY(hipMemcpyAsync(t.leaves.ptr, leaves ? (const void *)leaves : d_leaves, leaf_bytes, leaves ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice,
                                   ws.stream));
            in = t.leaves.ptr;
        } else if ((rc = stage_input(ws, ws.h2d_scalars, leaves, d_leaves, leaf_bytes, {After::STREAM, caller}, &in))) {
            return rc;
        }
        if ((rc = merkle_build(E, ws.stream, t, (const Fr *)in))) return rc;
        HIP_TRY(hipStreamSynchronize(ws.stream));
        return GMSM_OK;
    }
    // The levels of t (its shape set, t.nodes large enough) over the leaves at `in`, and the copy of the root to the host, queued
    // on s: what gmsm_merkle_new runs over the caller's leaves and a FRI oracle (gmsm_fri.h) over each of its layers.
    static int merkle_build(const char *E, hipStream_t s, MerkleTree &t, const Fr *in) {
        int rc;
        Fr *level = (Fr *)t.nodes.ptr;
        if ((rc = batch_launch(E, s, in, t.n, t.leaf_len, t.leaf_len, Fr::zero(), level))) return rc;
        size_t size = t.n;
        for (; size > MERKLE_TOP; level += size, size = (size + 1) / 2) {
            unsigned blocks;
            if ((rc = grid(E, (size + 1) / 2, &blocks))) return rc;
            hipLaunchKernelGGL((k_merkle_level<FrP>), dim3(blocks), dim3(MIMC_TPB), 0, s, (const Fr *)level, size, level + size);
        }
        if (size > 1) hipLaunchKernelGGL((k_merkle_top<FrP>), dim3(1), dim3(MIMC_TPB), 0, s, level, size);
        HIP_TRY(hipGetLastError());
        t.root.resize(sizeof(Fr) / 8);
        HIP_TRY(hipMemcpyAsync(t.root.data(), (const Fr *)t.nodes.ptr + (t.total - 1), sizeof(Fr), hipMemcpyDeviceToHost, s));
        return GMSM_OK;
    }

    // k > 0 paths, every index below n; out_leaves only with kept leaves (the engine has refused the rest)
    static int merkle_prove(Context &ctx, MerkleTree *tree, const uint64_t *indices, size_t k, uint64_t *out_leaves, uint64_t *out_siblings,
                            uint32_t *out_counts) {
        const char *E = "gmsm_merkle_prove";
        MerkleTree &t = *tree;
        GMSM_LEASE_OR_FAIL(lease, ctx);
        Workspace &ws = *lease.w;
        const size_t sib_bytes = k * t.depth * sizeof(Fr), leaf_bytes = out_leaves ? k * t.leaf_len * sizeof(Fr) : 0;
        const size_t cnt_at = sib_bytes + leaf_bytes, idx_at = (cnt_at + k * sizeof(uint32_t) + 15) & ~(size_t)15;
        int rc = ws.poly.ensure(idx_at + k * sizeof(uint64_t));
        if (rc) return rc;
        unsigned char *buf = (unsigned char *)ws.poly.ptr;
        unsigned blocks;
        if ((rc = grid(E, k, &blocks))) return rc;
        DrainOnExit drain{ws.stream};
        HIP_TRY(hipMemcpyAsync(buf + idx_at, indices, k * sizeof(uint64_t), hipMemcpyHostToDevice, ws.stream));
        hipLaunchKernelGGL((k_merkle_prove<FrP>), dim3(blocks), dim3(MIMC_TPB), 0, ws.stream, (const Fr *)t.nodes.ptr, t.n, t.depth,
                           out_leaves ? (const Fr *)t.leaves.ptr : nullptr, t.leaf_len, (const unsigned long long *)(buf + idx_at), k, (Fr *)buf,
                           (uint32_t *)(buf + cnt_at), (Fr *)(buf + sib_bytes));
        HIP_TRY(hipGetLastError());
        if (sib_bytes) HIP_TRY(hipMemcpyAsync(out_siblings, buf, sib_bytes, hipMemcpyDeviceToHost, ws.stream));
        if (leaf_bytes) HIP_TRY(hipMemcpyAsync(out_leaves, buf + sib_bytes, leaf_bytes, hipMemcpyDeviceToHost, ws.stream));
        HIP_TRY(hipMemcpyAsync(out_counts, buf + cnt_at, k * sizeof(uint32_t), hipMemcpyDeviceToHost, ws.stream));
        HIP_TRY(hipStreamSynchronize(ws.stream));
        return GMSM_OK;
    }
};

}  // namespace gmsm
