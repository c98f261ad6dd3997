// fr/polynomial.MultiLin and the sumcheck claim of one GKR wire on the device: the prover side of the reference's second
// proving stack (fr/polynomial, fr/sumcheck, fr/gkr), whose hot loop is data-parallel over the circuit's instances.
//
// Replaces, with identical results (every output is a uniquely determined element of Fr, stored canonically in Montgomery
// form; a field sum does not depend on its order, so any reduction shape gives the reference's bytes):
//   (*MultiLin).Fold, (MultiLin).Evaluate, (*MultiLin).Eq     ecc/bn254/fr/polynomial/multilin.go:21-40, 60-80, 150-172
//   eqTimesGateEvalSumcheckClaims.Combine / eqAcc / computeGJ / Next / ProveFinalEval   ecc/bn254/fr/gkr/gkr.go:143-348
// and the twins of BLS12-381 and BW6-761 (same templates, other scalar fields).
//
// Index convention (multilin.go:14-17): variable X_1 is the most significant bit of an index, so folding X_1 = r pairs
// element i with element i + len / 2.
//
// A Gate is a Go closure; here it is the straight-line program of gmsm_iop_expr.h (GMSM_EXPR_*, validated by the same
// host code), run by a second interpreter: k_gkr_round evaluates it at degree + 1 points per instance and reduces.
//
// Shape on the GPU:
//   k_multilin_fold        one lane per element of the lower half.
//   k_multilin_eq_table    the eq table of a few variables in closed form, one lane per entry: scale x the product of q_i or
//   k_multilin_eq_product  1 - q_i by the bits of the index. A table over n variables is the outer product of one over the
//                          high ceil(n/2) variables and one over the low floor(n/2): two tiny tables, then ONE product per
//                          output element (the reference's doubling loop makes n dependent passes over the table).
//   k_gkr_round            fold and round polynomial in one pass. With tables T_0 = E, T_1 .. T_m of length L, lane i < L / 4
//                          reads the slots i, i + L/4, i + L/2, i + 3L/4 of every table and writes the folded slots i and
//                          i + L/4 in place: no other lane touches those two, so the fold needs no barrier. Then, for
//                          d = 0 .. degree, the gate program runs on f_t(d) = T_t[i + half] + d (T_t[i + half] - T_t[i]).
//                          The program's register file lives in LDS as in k_iop_expr ([reg][16-byte piece][lane]); the
//                          operands are NOT kept there: an INPUT instruction reloads its two slots (the lane's own, L2- or
//                          L1-resident) and walks d steps, d additions against the products of the gate. With the operands
//                          in LDS an 8-input gate with 16 registers of BW6-761 elements would not fit 64 lanes; without,
//                          every valid program fits, so no claim is refused for its size. The lanes' values of one point
//                          are summed per wave with cross-lane moves, per workgroup through one more LDS row (slot
//                          [point][wave]: no barrier inside the point loop, one after it), and stored as
//                          [workgroup][degree + 1].
//   k_gkr_finish           one workgroup sums the workgroups' partial sums; the hand-off is the kernel boundary (no flag, no
//                          spin, no atomic). A round of one workgroup needs no second launch.
//   k_gkr_final            the last fold of the m input tables (length 2), element 0 of each.
#pragma once
#include <hip/hip_runtime.h>
#include "gmsm_context.h"
#include "gmsm_field.h"
#include "gmsm_fft.h"
#include "gmsm_iop_expr.h"

namespace gmsm {

constexpr unsigned GKR_TPB = EXPR_TPB;  // lanes of a workgroup; the round kernel halves it while its LDS exceeds EXPR_LDS_BYTES (expr_lanes_for)

// a[i] <- a[i] + r (a[i + half] - a[i]), i < half; the upper half is not written
template <class FrP>
__global__ void __launch_bounds__(GKR_TPB) k_multilin_fold(Fp<FrP> *a, size_t half, const Fp<FrP> r) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= half) return;
    const Fp<FrP> lo = fft_load(a, i);
    fft_store(a, i, fp_add(lo, fp_mul_inline(r, fp_sub(fft_load(a, i + half), lo))));
}

// out[h] = scale prod_{i < count} (bit_{count-1-i}(h) ? q[i] : 1 - q[i]), h < 2^count (count <= 32)
template <class FrP>
__global__ void __launch_bounds__(GKR_TPB) k_multilin_eq_table(const Fp<FrP> *q, unsigned count, const Fp<FrP> scale, Fp<FrP> *out) {
    using Fr = Fp<FrP>;
    const size_t h = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (h >> count) return;
    Fr v = scale;
#pragma nounroll
    for (unsigned i = 0; i < count; ++i) {
        const Fr qi = fft_load(q, i);  // uniform
        v = fp_mul_inline(v, ((h >> (count - 1 - i)) & 1) ? qi : fp_sub(Fr::one(), qi));
    }
    fft_store(out, h, v);
}

// out[h] (+)= hi[h >> nlo] lo[h & (2^nlo - 1)], h < total
template <class FrP>
__global__ void __launch_bounds__(GKR_TPB) k_multilin_eq_product(const Fp<FrP> *hi, const Fp<FrP> *lo, unsigned nlo, size_t total, int accumulate,
                                                                 Fp<FrP> *out) {
    const size_t h = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= total) return;
    Fp<FrP> v = fp_mul_inline(fft_load(hi, h >> nlo), fft_load(lo, h & (((size_t)1 << nlo) - 1)));
    if (accumulate) v = fp_add(v, fft_load(out, h));
    fft_store(out, h, v);
}

template <class FrP>
struct GkrRoundArgs {
    Fp<FrP> *tables;         // m + 1 tables, `stride` elements apart; table 0 is E
    size_t stride;
    size_t half;             // half the length the tables have when the program runs (after the fold, if any)
    const uint32_t *prog;    // validated: every opcode known, no POINT, inputs < m, constants in range, reads after writes
    const Fp<FrP> *consts;
    Fp<FrP> *partials;       // [gridDim.x][degree + 1]
    uint32_t prog_len, m, degree, fold, nregs, pad;
    Fp<FrP> r;               // the fold's challenge
};

// T[i + half] + d (T[i + half] - T[i]): T at X = d + 1 on the line through T(0) = T[i], T(1) = T[i + half]
template <class Fr>
__device__ __forceinline__ Fr gkr_operand(const Fr *t, size_t i, size_t half, unsigned d) {
    const Fr hi = fft_load(t, i + half);
    const Fr step = fp_sub(hi, fft_load(t, i));
    Fr v = hi;
#pragma nounroll
    for (unsigned k = 0; k < d; ++k) v = fp_add(v, step);  // d is uniform and at most GMSM_GKR_MAX_DEGREE
    return v;
}

// Dynamic LDS: (nregs + 1) x sizeof(Fr) x blockDim.x bytes; blockDim.x is a multiple of 64. Every lane reaches the one barrier.
template <class FrP>
__global__ void __launch_bounds__(GKR_TPB) k_gkr_round(const GkrRoundArgs<FrP> args) {
    using Fr = Fp<FrP>;
    static_assert(sizeof(Fr) % 16 == 0, "element size");
    extern __shared__ __align__(16) unsigned char gkr_lds_raw[];
    uint4 *regs = reinterpret_cast<uint4 *>(gkr_lds_raw);
    const unsigned lane = threadIdx.x, lanes = blockDim.x, waves = lanes >> 6, npts = args.degree + 1;
    const size_t i = (size_t)blockIdx.x * lanes + lane, half = args.half;
    const bool active = i < half;
    if (active && args.fold) {
#pragma nounroll
        for (unsigned t = 0; t <= args.m; ++t) {
            Fr *T = args.tables + (size_t)t * args.stride;  // old length 4 half: X_1 pairs i with i + 2 half
            const Fr a0 = fft_load(T, i), a1 = fft_load(T, i + half);
            const Fr lo = fp_add(a0, fp_mul_inline(args.r, fp_sub(fft_load(T, i + 2 * half), a0)));
            const Fr hi = fp_add(a1, fp_mul_inline(args.r, fp_sub(fft_load(T, i + 3 * half), a1)));
            fft_store(T, i, lo);
            fft_store(T, i + half, hi);
        }
    }
#pragma nounroll
    for (unsigned d = 0; d < npts; ++d) {
        Fr v = Fr::zero();
        if (active) {
#pragma nounroll
            for (uint32_t pc = 0; pc < args.prog_len; ++pc) {
                const uint32_t ins = args.prog[pc];  // uniform: a scalar load
                const unsigned op = ins & 0xff, dst = (ins >> 8) & 0xff, a = (ins >> 16) & 0xff, b = ins >> 24;
                switch (op) {
                    case GMSM_EXPR_INPUT: v = gkr_operand(args.tables + (size_t)(a + 1) * args.stride, i, half, d); break;
                    case GMSM_EXPR_CONST: v = args.consts[a]; break;
                    case GMSM_EXPR_ADD: v = fp_add(expr_reg_read<Fr>(regs, a, lanes, lane), expr_reg_read<Fr>(regs, b, lanes, lane)); break;
                    case GMSM_EXPR_SUB: v = fp_sub(expr_reg_read<Fr>(regs, a, lanes, lane), expr_reg_read<Fr>(regs, b, lanes, lane)); break;
                    case GMSM_EXPR_MUL: v = fp_mul_inline(expr_reg_read<Fr>(regs, a, lanes, lane), expr_reg_read<Fr>(regs, b, lanes, lane)); break;
                    default: v = fp_neg(expr_reg_read<Fr>(regs, a, lanes, lane)); break;  // GMSM_EXPR_NEG
                }
                expr_reg_write(regs, dst, lanes, lane, v);
            }
            v = fp_mul_inline(gkr_operand(args.tables, i, half, d), v);
        }
        // the wave's sum, in its lane 0
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            Fr o;
#pragma unroll
            for (int k = 0; k < Fr::N; ++k) o.l[k] = (uint32_t)__shfl_down((int)v.l[k], off, 64);
            v = fp_add(v, o);
        }
        if ((lane & 63) == 0) expr_reg_write(regs, args.nregs, lanes, d * waves + (lane >> 6), v);  // npts waves <= 16 waves <= lanes
    }
    __syncthreads();
    if (lane < npts) {
        Fr s = expr_reg_read<Fr>(regs, args.nregs, lanes, lane * waves);
        for (unsigned w = 1; w < waves; ++w) s = fp_add(s, expr_reg_read<Fr>(regs, args.nregs, lanes, lane * waves + w));
        fft_store(args.partials, (size_t)blockIdx.x * npts + lane, s);
    }
}

// out[d] = sum_b partials[b npts + d]: one workgroup of GKR_TPB lanes, a tree in LDS per point
template <class FrP>
__global__ void __launch_bounds__(GKR_TPB) k_gkr_finish(const Fp<FrP> *partials, size_t blocks, unsigned npts, Fp<FrP> *out) {
    using Fr = Fp<FrP>;
    __shared__ Fr tree[GKR_TPB];
    const unsigned l = threadIdx.x;
    for (unsigned d = 0; d < npts; ++d) {
        Fr s = Fr::zero();
        for (size_t b = l; b < blocks; b += GKR_TPB) s = fp_add(s, fft_load(partials, b * npts + d));
        tree[l] = s;
        __syncthreads();
        for (unsigned w = GKR_TPB / 2; w > 0; w >>= 1) {
            if (l < w) tree[l] = fp_add(tree[l], tree[l + w]);
            __syncthreads();
        }
        if (l == 0) fft_store(out, d, tree[0]);
        __syncthreads();
    }
}

// out[t] = T_(t+1)[0] + r (T_(t+1)[1] - T_(t+1)[0]), t < m: ProveFinalEval's fold of the length-2 input tables
template <class FrP>
__global__ void __launch_bounds__(64) k_gkr_final(const Fp<FrP> *tables, size_t stride, unsigned m, const Fp<FrP> r, Fp<FrP> *out) {
    const unsigned t = threadIdx.x;
    if (t >= m) return;
    const Fp<FrP> *T = tables + (size_t)(t + 1) * stride;
    const Fp<FrP> lo = fft_load(T, 0);
    fft_store(out, t, fp_add(lo, fp_mul_inline(r, fp_sub(fft_load(T, 1), lo))));
}

// ------------------------------------------------------------------ host side of one scalar field
template <class FrP>
struct GkrField {
    using Fr = Fp<FrP>;

    static int grid(const char *E, size_t n, unsigned tpb, unsigned *blocks) {
        const size_t b = (n + tpb - 1) / tpb;
        if (b > 0x7fffffffu) return fail(GMSM_ERR_ARG, std::string(E) + ": len is too large for one launch");
        *blocks = (unsigned)b;
        return GMSM_OK;
    }

    static int fold_launch(const char *E, hipStream_t s, Fr *a, size_t len, const Fr &r) {
        unsigned blocks;
        if (int rc = grid(E, len / 2, GKR_TPB, &blocks)) return rc;
        hipLaunchKernelGGL((k_multilin_fold<FrP>), dim3(blocks), dim3(GKR_TPB), 0, s, a, len / 2, r);
        HIP_TRY(hipGetLastError());
        return GMSM_OK;
    }

    // out[h] (+)= scale eq(q, h) for h < 2^n. d_q: n elements on the device; scratch: eq_scratch(n) elements
    static size_t eq_scratch(unsigned n) { return ((size_t)1 << ((n + 1) / 2)) + ((size_t)1 << (n / 2)); }
    static int eq_launch(const char *E, hipStream_t s, const Fr *d_q, unsigned n, const Fr &scale, bool accumulate, Fr *scratch, Fr *out) {
        const unsigned nhi = (n + 1) / 2, nlo = n / 2;
        Fr *hi = scratch, *lo = scratch + ((size_t)1 << nhi);
        unsigned blocks;
        int rc;
        if ((rc = grid(E, (size_t)1 << nhi, GKR_TPB, &blocks))) return rc;
        hipLaunchKernelGGL((k_multilin_eq_table<FrP>), dim3(blocks), dim3(GKR_TPB), 0, s, d_q, nhi, scale, hi);
        if ((rc = grid(E, (size_t)1 << nlo, GKR_TPB, &blocks))) return rc;
        hipLaunchKernelGGL((k_multilin_eq_table<FrP>), dim3(blocks), dim3(GKR_TPB), 0, s, d_q + nhi, nlo, Fr::one(), lo);
        if ((rc = grid(E, (size_t)1 << n, GKR_TPB, &blocks))) return rc;
        hipLaunchKernelGGL((k_multilin_eq_product<FrP>), dim3(blocks), dim3(GKR_TPB), 0, s, (const Fr *)hi, (const Fr *)lo, nlo, (size_t)1 << n,
                           accumulate ? 1 : 0, out);
        HIP_TRY(hipGetLastError());
        return GMSM_OK;
    }

    // ---- the three MultiLin entries: a leased workspace, its stream ordered after the caller's
    static int multilin_fold(Context &ctx, uint64_t *a, void *d_a, size_t len, const uint64_t *r, hipStream_t caller) {
        const char *E = "gmsm_multilin_fold";
        GMSM_LEASE_OR_FAIL(lease, ctx);
        Workspace &ws = *lease.w;
        void *v;
        DrainOnExit drain{ws.stream};
        int rc = stage_input(ws, ws.h2d_scalars, a, d_a, len * sizeof(Fr), {After::STREAM, caller}, &v);
        if (rc || (rc = fold_launch(E, ws.stream, (Fr *)v, len, fr_from_limbs<Fr>(r)))) return rc;
        if (a) HIP_TRY(hipMemcpyAsync(a, v, len / 2 * sizeof(Fr), hipMemcpyDeviceToHost, ws.stream));  // the upper half stays as it was
        HIP_TRY(hipStreamSynchronize(ws.stream));
        return GMSM_OK;
    }
    static int multilin_evaluate(Context &ctx, const uint64_t *m, const void *d_m, size_t len, const uint64_t *coords, size_t ncoords,
                                 hipStream_t caller, uint64_t *out_value) {
        const char *E = "gmsm_multilin_evaluate";
        GMSM_LEASE_OR_FAIL(lease, ctx);
        Workspace &ws = *lease.w;
        int rc;
        if (d_m && (rc = order_after(ws, caller))) return rc;
        const size_t need = ncoords ? len : 1;  // no fold: only element 0 is read
        if ((rc = ws.poly.ensure(need * sizeof(Fr)))) return rc;
        Fr *v = (Fr *)ws.poly.ptr;
        DrainOnExit drain{ws.stream};
        HIP_TRY(hipMemcpyAsync(v, m ? (const void *)m : d_m, need * sizeof(Fr), m ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, ws.stream));
        for (size_t j = 0; j < ncoords; ++j)  // back to back: the stream orders them
            if ((rc = fold_launch(E, ws.stream, v, len >> j, fr_from_limbs<Fr>(coords + j * (sizeof(Fr) / 8))))) return rc;
        HIP_TRY(hipMemcpyAsync(out_value, v, sizeof(Fr), hipMemcpyDeviceToHost, ws.stream));
        HIP_TRY(hipStreamSynchronize(ws.stream));
        return GMSM_OK;
    }
    static int multilin_eq(Context &ctx, const uint64_t *q, unsigned n, const uint64_t *scale, int accumulate, hipStream_t caller, uint64_t *out,
                           void *d_out) {
        const char *E = "gmsm_multilin_eq";
        GMSM_LEASE_OR_FAIL(lease, ctx);
        Workspace &ws = *lease.w;
        const size_t total = (size_t)1 << n;
        int rc;
        if (d_out && (rc = order_after(ws, caller))) return rc;  // the caller's stream may still use d_out
        if ((rc = ws.poly.ensure((n + eq_scratch(n)) * sizeof(Fr)))) return rc;
        if (out && (rc = ws.h2d_scalars.ensure(total * sizeof(Fr)))) return rc;
        Fr *dq = (Fr *)ws.poly.ptr, *res = out ? (Fr *)ws.h2d_scalars.ptr : (Fr *)d_out;
        DrainOnExit drain{ws.stream};
        if (n) HIP_TRY(hipMemcpyAsync(dq, q, n * sizeof(Fr), hipMemcpyHostToDevice, ws.stream));
        if (out && accumulate) HIP_TRY(hipMemcpyAsync(res, out, total * sizeof(Fr), hipMemcpyHostToDevice, ws.stream));
        if ((rc = eq_launch(E, ws.stream, dq, n, fr_from_limbs<Fr>(scale), accumulate != 0, dq + n, res))) return rc;
        if (out) HIP_TRY(hipMemcpyAsync(out, res, total * sizeof(Fr), hipMemcpyDeviceToHost, ws.stream));
        HIP_TRY(hipStreamSynchronize(ws.stream));
        return GMSM_OK;
    }

    // ---- one sumcheck claim (GkrClaim, gmsm_context.h): its tables and small buffers are its own, its rounds run on its stream
    static size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }

    // the round polynomial of the claim's tables, after folding them by r when fold is set; out_gj: degree + 1 elements (host)
    static int round(const char *E, GkrClaim &c, bool fold, const Fr &r, uint64_t *out_gj) {
        const size_t half = fold ? c.len / 4 : c.len / 2;
        unsigned lanes = c.lanes;
        while (lanes > 64 && lanes / 2 >= half) lanes >>= 1;  // a short round does not launch idle waves
        unsigned blocks;
        if (int rc = grid(E, half, lanes, &blocks)) return rc;
        unsigned char *small = (unsigned char *)c.small.ptr;
        GkrRoundArgs<FrP> args;
        args.tables = (Fr *)c.tables.ptr, args.stride = c.stride, args.half = half;
        args.prog = (const uint32_t *)(small + c.prog_at), args.consts = (const Fr *)small, args.partials = (Fr *)(small + c.partials_at);
        args.prog_len = c.prog_len, args.m = (uint32_t)c.m, args.degree = (uint32_t)c.degree, args.fold = fold ? 1u : 0u, args.nregs = c.nregs, args.pad = 0;
        args.r = r;
        const unsigned npts = (unsigned)c.degree + 1;
        DrainOnExit drain{c.stream};
        hipLaunchKernelGGL((k_gkr_round<FrP>), dim3(blocks), dim3(lanes), (size_t)(c.nregs + 1) * sizeof(Fr) * lanes, c.stream, args);
        HIP_TRY(hipGetLastError());
        if (fold) c.len /= 2;
        const Fr *res = args.partials;  // one workgroup: its partial sums are the sums
        if (blocks > 1) {
            Fr *sum = (Fr *)(small + c.result_at);
            hipLaunchKernelGGL((k_gkr_finish<FrP>), dim3(1), dim3(GKR_TPB), 0, c.stream, (const Fr *)args.partials, (size_t)blocks, npts, sum);
            HIP_TRY(hipGetLastError());
            res = sum;
        }
        HIP_TRY(hipMemcpyAsync(out_gj, res, npts * sizeof(Fr), hipMemcpyDeviceToHost, c.stream));
        HIP_TRY(hipStreamSynchronize(c.stream));
        return GMSM_OK;
    }

    // The engine has validated everything and set the claim's shape (group, device, stream, m, degree, stride = len, nregs,
    // prog_len); here: its memory, the copies of the tables, E = sum_j comb^j eq(points[j], .), the first round polynomial.
    static int gkr_new(Context &ctx, GkrClaim *claim, const uint32_t *prog, const uint64_t *consts, size_t n_consts, const uint64_t *const *tables,
                       const void *const *d_tables, const uint64_t *points, size_t k, const uint64_t *comb, uint64_t *out_gj) {
        const char *E = "gmsm_gkr_claim_new";
        GkrClaim &c = *claim;
        (void)ctx;
        unsigned n = 0;
        while (((size_t)1 << n) < c.stride) ++n;
        // the round kernel's workgroup: register file and row of wave sums within EXPR_LDS_BYTES (16 registers: 64 lanes; MiMC's three: 256)
        c.lanes = expr_lanes_for<Fr>(c.nregs + 1);
        const size_t max_blocks = (c.stride / 2 + 63) / 64, npts = c.degree + 1;
        c.prog_at = n_consts * sizeof(Fr);
        c.partials_at = c.prog_at + align16(c.prog_len * sizeof(uint32_t));
        c.result_at = c.partials_at + max_blocks * npts * sizeof(Fr);
        const size_t q_at = c.result_at + std::max(npts, c.m) * sizeof(Fr), scratch_at = q_at + k * n * sizeof(Fr);
        int rc;
        if ((rc = c.small.ensure(scratch_at + eq_scratch(n) * sizeof(Fr))) || (rc = c.tables.ensure((c.m + 1) * c.stride * sizeof(Fr)))) return rc;
        unsigned char *small = (unsigned char *)c.small.ptr;
        Fr *T = (Fr *)c.tables.ptr;
        DrainOnExit drain{c.stream};
        if (n_consts) HIP_TRY(hipMemcpyAsync(small, consts, n_consts * sizeof(Fr), hipMemcpyHostToDevice, c.stream));
        HIP_TRY(hipMemcpyAsync(small + c.prog_at, prog, c.prog_len * sizeof(uint32_t), hipMemcpyHostToDevice, c.stream));
        if (n) HIP_TRY(hipMemcpyAsync(small + q_at, points, k * n * sizeof(Fr), hipMemcpyHostToDevice, c.stream));
        for (size_t t = 0; t < c.m; ++t)  // copies: folding destroys them, and the caller's are never modified
            HIP_TRY(hipMemcpyAsync(T + (t + 1) * c.stride, tables ? (const void *)tables[t] : d_tables[t], c.stride * sizeof(Fr),
                                   tables ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, c.stream));
        Fr scale = Fr::one();
        for (size_t j = 0; j < k; ++j) {
            if (j) scale = fp_mul(scale, fr_from_limbs<Fr>(comb));
            if ((rc = eq_launch(E, c.stream, (const Fr *)(small + q_at) + j * n, n, scale, j != 0, (Fr *)(small + scratch_at), T))) return rc;
        }
        return round(E, c, false, Fr::zero(), out_gj);
    }
    static int gkr_next(GkrClaim *claim, const uint64_t *r, uint64_t *out_gj) { return round("gmsm_gkr_claim_next", *claim, true, fr_from_limbs<Fr>(r), out_gj); }
    static int gkr_final(GkrClaim *claim, const uint64_t *r, uint64_t *out_evals) {
        GkrClaim &c = *claim;
        Fr *res = (Fr *)((unsigned char *)c.small.ptr + c.result_at);
        DrainOnExit drain{c.stream};
        hipLaunchKernelGGL((k_gkr_final<FrP>), dim3(1), dim3(64), 0, c.stream, (const Fr *)c.tables.ptr, c.stride, (unsigned)c.m, fr_from_limbs<Fr>(r), res);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(out_evals, res, c.m * sizeof(Fr), hipMemcpyDeviceToHost, c.stream));
        HIP_TRY(hipStreamSynchronize(c.stream));
        return GMSM_OK;
    }
};

}  // namespace gmsm
