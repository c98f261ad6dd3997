// iop.Evaluate on the device: a multivariate expression applied index by index to m polynomials of equal length - how a
// PLONK prover makes its constraint numerator on the big coset between ToLagrangeCoset and DivideByXMinusOne
// (gmsm_iop_poly.h), without taking the wire polynomials back to the host.
//
// Replaces, with identical results (every output is a uniquely determined element of Fr, stored canonically in Montgomery
// form):
//   Evaluate(f Expression, r, form, x ...*Polynomial)     ecc/bn254/fr/iop/expressions.go:26-73
//   (*Polynomial).GetCoeff                                polynomial.go:151-163 (the read of x_j at index i)
// and the twins of BLS12-381 and BW6-761 (same templates, other scalar fields).
//
// A Go closure cannot run here. An expression of this kind is a fixed sequence of field additions, subtractions and
// products, the same for every index: a straight-line program (format: include/gmsm.h, GMSM_EXPR_*), validated on the host
// (gmsm_engine.hip) so that the kernel never sees a bad one, and interpreted by ONE kernel, one index per lane, with no flag,
// spin or barrier - not even inside a workgroup: a lane touches nothing but its own slots.
//
// Shape on the GPU:
//   k_iop_expr   lane i of the grid owns index i. The program, the constants and the input descriptors sit in one small
//                device buffer and are indexed by values that are uniform over the grid, so fetch and decode are scalar.
//                The register file is in LDS, not in a per-lane array (an array indexed by a run-time register number
//                lands in scratch memory): [reg][16-byte piece][lane], so the lanes of a wave touch consecutive 16-byte
//                pieces (one conflict-free ds_read_b128 / ds_write_b128 per piece), sized by the registers the program
//                really uses x the element size x the lanes of the workgroup. The workgroup shrinks from 256 lanes until
//                its file fits EXPR_LDS_BYTES (a 16-register BN254 program: 128 lanes, BW6-761 with its 48-byte elements: 64),
//                so that two workgroups always share a CU and a three-register program keeps 24 waves there.
//                Arithmetic is the canonical fp_add / fp_sub / fp_neg and fp_mul's body inlined (fp_mul_inline: a call would pass
//                the second operand of a 12-limb product through scratch memory). The value of the last instruction stays
//                in VGPRs and is stored once; a slot the output shares with an input (same layout, offset 0) was read by
//                the lane that writes it.
//   POINT        w^i from the domain's resident twiddles 2^s w^k, k < len / 2 (lazy domain, gmsm_fft_lazy.h), as
//                ratio_omega reads them, times 2^-s: one load and one product; 1 for len = 1, which has no table.
#pragma once
#include <hip/hip_runtime.h>
#include "gmsm_context.h"
#include "gmsm_field.h"
#include "gmsm_fft.h"
#include "gmsm_ratio.h"

namespace gmsm {

// the opcodes and limits of a program are the header's (include/gmsm.h: GMSM_EXPR_*)
constexpr unsigned EXPR_TPB = 256;             // lanes of a workgroup, halved while the register file exceeds:
constexpr size_t EXPR_LDS_BYTES = 64 * 1024;   // two workgroups per CU at the least, and no opt-in to large dynamic LDS

// One input polynomial as the kernel sees it: where it starts, the offset rho_j shift_j mod len of its reads, its layout
struct ExprInput {
    const void *ptr;
    uint64_t offset;  // < len
    uint32_t rev;     // 1: BitReverse
    uint32_t pad;
};

template <class FrP>
struct ExprArgs {
    const uint32_t *prog;     // prog_len words
    const Fp<FrP> *consts;    // canonical Montgomery elements
    const ExprInput *inputs;  // m descriptors
    const Fp<FrP> *tw;        // POINT: 2^s w^k, k < len / 2; null without POINT or for len = 1
    Fp<FrP> *out;             // may be one of the inputs (same layout, offset 0)
    size_t len;
    uint32_t prog_len, log2len, out_rev, pad;
    Fp<FrP> unshift;          // 2^-s
};

// slot (reg, lane) of the register file: piece p at regs[(reg * PIECES + p) * lanes + lane]
template <class Fr>
__device__ __forceinline__ Fr expr_reg_read(const uint4 *regs, unsigned reg, unsigned lanes, unsigned lane) {
    constexpr unsigned PIECES = sizeof(Fr) / 16;
    Fr r;
    uint4 *dst = reinterpret_cast<uint4 *>(&r);
#pragma unroll
    for (unsigned p = 0; p < PIECES; ++p) dst[p] = regs[(reg * PIECES + p) * lanes + lane];
    return r;
}
template <class Fr>
__device__ __forceinline__ void expr_reg_write(uint4 *regs, unsigned reg, unsigned lanes, unsigned lane, const Fr &v) {
    constexpr unsigned PIECES = sizeof(Fr) / 16;
    const uint4 *src = reinterpret_cast<const uint4 *>(&v);
#pragma unroll
    for (unsigned p = 0; p < PIECES; ++p) regs[(reg * PIECES + p) * lanes + lane] = src[p];
}

// lanes of a workgroup whose LDS holds `rows` elements per lane (a program's register file; the GKR round adds a row of wave
// sums): 256, halved while that exceeds EXPR_LDS_BYTES (never below a wave: 16 registers of 48 bytes x 64 lanes = 48 KiB)
template <class Fr>
static inline unsigned expr_lanes_for(unsigned rows) {
    unsigned lanes = EXPR_TPB;
    while (lanes > 64 && (size_t)rows * sizeof(Fr) * lanes > EXPR_LDS_BYTES) lanes >>= 1;
    return lanes;
}

// out[idx(i)] = the program at index i = blockIdx.x * blockDim.x + threadIdx.x. Dynamic LDS: registers used x sizeof(Fr) x
// blockDim.x bytes. The host has validated the program: every opcode is known, every register read was written before,
// every input and constant index is in range, POINT comes with a table (or len = 1).
template <class FrP>
__global__ void __launch_bounds__(EXPR_TPB) k_iop_expr(const ExprArgs<FrP> args) {
    using Fr = Fp<FrP>;
    static_assert(sizeof(Fr) % 16 == 0, "element size");
    extern __shared__ __align__(16) unsigned char expr_lds_raw[];
    uint4 *regs = reinterpret_cast<uint4 *>(expr_lds_raw);
    const unsigned lane = threadIdx.x, lanes = blockDim.x;
    const size_t i = (size_t)blockIdx.x * lanes + lane;
    if (i >= args.len) return;  // no barrier anywhere below
    Fr r = Fr::zero();
#pragma nounroll
    for (uint32_t pc = 0; pc < args.prog_len; ++pc) {
        const uint32_t ins = args.prog[pc];  // uniform: a scalar load
        const unsigned op = ins & 0xff, dst = (ins >> 8) & 0xff, a = (ins >> 16) & 0xff, b = ins >> 24;
        switch (op) {
            case GMSM_EXPR_INPUT: {
                const ExprInput in = args.inputs[a];
                size_t s = i + in.offset;  // both below len
                if (s >= args.len) s -= args.len;
                r = fft_load(reinterpret_cast<const Fr *>(in.ptr), in.rev ? fft_bitrev(s, args.log2len) : s);
                break;
            }
            case GMSM_EXPR_CONST: r = args.consts[a]; break;
            case GMSM_EXPR_POINT:
                r = args.tw ? fp_mul_inline(ratio_omega(args.tw, i, args.len >> 1), args.unshift) : Fr::one();
                break;
            case GMSM_EXPR_ADD: r = fp_add(expr_reg_read<Fr>(regs, a, lanes, lane), expr_reg_read<Fr>(regs, b, lanes, lane)); break;
            case GMSM_EXPR_SUB: r = fp_sub(expr_reg_read<Fr>(regs, a, lanes, lane), expr_reg_read<Fr>(regs, b, lanes, lane)); break;
            case GMSM_EXPR_MUL: r = fp_mul_inline(expr_reg_read<Fr>(regs, a, lanes, lane), expr_reg_read<Fr>(regs, b, lanes, lane)); break;
            default: r = fp_neg(expr_reg_read<Fr>(regs, a, lanes, lane)); break;  // GMSM_EXPR_NEG
        }
        expr_reg_write(regs, dst, lanes, lane, r);
    }
    fft_store(args.out, args.out_rev ? fft_bitrev(i, args.log2len) : i, r);
}

// ------------------------------------------------------------------ host side of one scalar field
template <class FrP>
struct IopExprField {
    using Fr = Fp<FrP>;

    // Enqueues the one kernel. prog / consts / inputs: device; tw: the domain's twiddles_lz when the program has a POINT
    // and len > 1, else null.
    static int run(hipStream_t stream, const uint32_t *prog, size_t prog_len, unsigned nregs, const Fr *consts, const ExprInput *inputs,
                   const Fr *tw, size_t len, bool out_rev, Fr *out) {
        ExprArgs<FrP> args;
        args.prog = prog, args.consts = consts, args.inputs = inputs, args.tw = tw, args.out = out, args.len = len;
        args.prog_len = (uint32_t)prog_len, args.log2len = 0, args.out_rev = out_rev ? 1u : 0u, args.pad = 0;
        while (((size_t)1 << args.log2len) < len) ++args.log2len;  // read only where len is a power of two
        args.unshift = tw ? fp_inv(FftField<FrP>::lazy_shift()) : Fr::one();
        const unsigned lanes = expr_lanes_for<Fr>(nregs);
        const size_t blocks = (len + lanes - 1) / lanes;
        if (blocks > 0x7fffffffu) return fail(GMSM_ERR_ARG, "gmsm_iop_evaluate_expression: len is too large for one launch");
        hipLaunchKernelGGL((k_iop_expr<FrP>), dim3((unsigned)blocks), dim3(lanes), (size_t)nregs * sizeof(Fr) * lanes, stream, args);
        HIP_TRY(hipGetLastError());
        return GMSM_OK;
    }
};

}  // namespace gmsm
