// One (curve, group) instance of the engine: struct Group decides what a call runs as - the sorted-bucket pipeline of
// gmsm_pipeline.h (its base class, over the host-side arithmetic of gmsm_group_host.h), the fused small-n kernel, window
// tables, point ranges - and holds the group's other device entries. The test hooks live in gmsm_group_debug.h, the function table the C ABI dispatches through in
// gmsm_group_vtable.h (both included at the end). Instantiated once per group in gmsm_group_inst.hip (one translation
// unit per group so the six groups compile in parallel).
#pragma once
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <type_traits>
#include <vector>

#include "gmsm_pipeline.h"
#include "gmsm_small.h"
#include "gmsm_fixedbase.h"
#include "gmsm_ingest.h"
#include "gmsm_decompress.h"
#include "gmsm_fft.h"
#include "gmsm_poly.h"
#include "gmsm_shplonk.h"
#include "gmsm_fflonk.h"
#include "gmsm_group_fft.h"
#include "gmsm_scale.h"
#include "gmsm_ratio.h"
#include "gmsm_iop_poly.h"
#include "gmsm_iop_expr.h"
#include "gmsm_gkr.h"

namespace gmsm {

// ------------------------------------------------------------------ one (curve, group)
template <class F_, class FrP_, class Consts_, bool NEEDS_TORSION_>
struct Group : Pipeline<F_, FrP_, Consts_> {
    using Pipe = Pipeline<F_, FrP_, Consts_>;  // the sorted-bucket pipeline: plans, layout, stages, collection
    using Host = GroupHost<F_, FrP_>;          // fold, fold_sets, generate_points, build_fixed_base_table, fold_powers
    using Host::batch_to_affine, Host::build_fixed_base_table, Host::fold, Host::fold_planes, Host::fold_powers, Host::fold_sets;
    using Host::generate_points, Host::scalar_mul;
    using typename Pipe::Aff, typename Pipe::Consts, typename Pipe::Ext, typename Pipe::F, typename Pipe::FrP, typename Pipe::J;
    using typename Pipe::OpsSerial, typename Pipe::U;
    using Pipe::AFF_BYTES, Pipe::FR_BITS, Pipe::bucket_sets, Pipe::collect_folded, Pipe::collect_window_sums, Pipe::enqueue_reduce;
    using Pipe::enqueue_window_sums, Pipe::glv_width_built, Pipe::make_plan, Pipe::make_plan_glv;
    static constexpr bool NEEDS_TORSION = NEEDS_TORSION_;  // cofactor != 1: subgroup check beyond the curve equation
    static constexpr size_t SCALAR_BYTES = sizeof(Fp<FrP>);
    // fixed-base / normalisation / table-doubling kernels: every type inlines its group operations since the end of round 6 (the wide
    // types called theirs out of line through rounds 2-6 for code size: same-box A/B profiles/r06_fixed_base_inline_ab.log - BN254 G2
    // 2^20 17.7 -> 8.7 ms, BLS12-381 G2 34.4 -> 18.2, BW6-761 53.6 -> 36.1). -DGMSM_INLINE_OPS_BYTES=56 gives the old form back.
#ifndef GMSM_INLINE_OPS_BYTES
#define GMSM_INLINE_OPS_BYTES (28 * 4)
#endif
    static constexpr bool INLINE_OPS = sizeof(U) <= GMSM_INLINE_OPS_BYTES;
    static constexpr bool SKEWED_HOST_RANGES = AFF_BYTES <= 96;  // host_ranges / window_sums_from_host

    // Runs the device pipeline for the windows of `plan`; host_xyzz receives plan.nwin_local window totals.
    // d_points: Go-layout affine bases on the device, or nullptr when `resident` (bases already rewritten into the lazy
    // domain by register_bases) is given.
    // `ws` is leased by the caller; the pipeline runs on the workspace's own stream, ordered after `caller_stream`.
    static int window_sums(Context &ctx, Workspace &ws, const void *d_points, const void *d_scalars, size_t n,
                           const WindowPlan &plan, hipStream_t caller_stream, Ext *host_xyzz,
                           const ResidentBases *resident = nullptr, size_t resident_offset = 0) {
        int rc = order_after(ws, caller_stream);
        if (rc) return rc;
        RunRequest rq;
        rq.resident_offset = resident_offset;
        rq.tail_mode = TAIL_IF_FORCED;
        if ((rc = enqueue_window_sums(ctx, ws, d_points, d_scalars, n, plan, ws.stream, resident, rq))) return rc;
        return collect_window_sums(ws, ws.stream, plan.nwin_local, host_xyzz);
    }
    // The same for a caller that wants the folded MultiExp: the reduction may leave its scaling to the host fold.
    static int window_sums_folded(Context &ctx, Workspace &ws, const void *d_points, const void *d_scalars, size_t n,
                                  const WindowPlan &plan, hipStream_t caller_stream, J *out, const ResidentBases *resident) {
        int rc = order_after(ws, caller_stream);
        if (rc) return rc;
        RunRequest rq;
        rq.tail_mode = TAIL_AUTO;
        if ((rc = enqueue_window_sums(ctx, ws, d_points, d_scalars, n, plan, ws.stream, resident, rq))) return rc;
        return collect_folded(ws, ws.stream, plan.c, plan.nwin_total, out);
    }

    // ---- N3: fixed-base batch scalar multiplication / batch normalisation (gmsm_fixedbase.h; the table is GroupHost's) ----
    // recs (lazy XYZZ records, n of them, already on the device in ws.buckets) -> d_out affine; K records per thread
    static int normalize_records(Workspace &ws, size_t n, void *d_out) {
        int rc;
        if ((rc = ws.partials.ensure(n * sizeof(U)))) return rc;
        constexpr int K = 32;
        const size_t threads = (n + K - 1) / K;
        hipLaunchKernelGGL((k_batch_normalize<U, INLINE_OPS, K>), dim3((unsigned)((threads + 63) / 64)), dim3(64), 0, ws.stream,
                           ws.buckets.ptr, n, (U *)ws.partials.ptr, d_out);
        HIP_TRY(hipGetLastError());
        return GMSM_OK;
    }

    // BatchScalarMultiplicationG1 (g1.go:1039): out[i] = scalars[i] * base, affine. d_scalars/d_out on the device.
    static int batch_scalar_mul(Context &ctx, Workspace &ws, const uint64_t *base_limbs, const void *d_scalars, size_t n,
                                void *d_out) {
        if (n == 0) return GMSM_OK;
        Aff base;
        memcpy(&base, base_limbs, sizeof base);
        if (base.is_infinity()) {
            HIP_TRY(hipMemsetAsync(d_out, 0, n * AFF_BYTES, ws.stream));
            return GMSM_OK;
        }
        // table size against additions per scalar: 2^7 x 32 windows up to 2^21 scalars, 2^10 x 24 beyond (BN254)
        const unsigned forced_c = options().fixed_base_bits.load(std::memory_order_relaxed);
        const unsigned c = forced_c ? forced_c : n < ((size_t)1 << 21) ? 8 : 11;
        const WindowPlan plan = make_plan(c, 0, 1);
        std::vector<Aff> table;
        build_fixed_base_table(base, plan.c, plan.nwin_total, plan.nbuckets, (int)std::min<unsigned>(16, usable_cpus()), table);
        int rc;
        const size_t tn = table.size();
        if ((rc = ws.h2d_points.ensure(tn * AFF_BYTES))) return rc;
        if ((rc = ws.upoints.ensure(tn * AFF_BYTES))) return rc;
        if ((rc = ws.skip.ensure(tn))) return rc;
        if ((rc = ws.buckets.ensure(n * sizeof(XYZZL<U>)))) return rc;
        HIP_TRY(hipMemcpyAsync(ws.h2d_points.ptr, table.data(), tn * AFF_BYTES, hipMemcpyHostToDevice, ws.stream));
        hipLaunchKernelGGL((k_convert_points<U>), dim3((unsigned)((tn + 255) / 256)), dim3(256), 0, ws.stream,
                           ws.h2d_points.ptr, tn, ws.upoints.ptr, (uint8_t *)ws.skip.ptr);
        hipLaunchKernelGGL((k_fixed_base<U, FrP, INLINE_OPS>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ws.stream,
                           (const uint32_t *)d_scalars, n, plan, ws.upoints.ptr, ws.buckets.ptr);
        HIP_TRY(hipGetLastError());
        if ((rc = normalize_records(ws, n, d_out))) return rc;
        HIP_TRY(hipStreamSynchronize(ws.stream));  // `table` (pageable host memory) must outlive the copy
        return GMSM_OK;
    }

    // BatchJacobianToAffineG1 (g1.go:989): d_jac = n Go-layout Jacobian points on the device -> d_out affine
    static int batch_jac_to_affine(Workspace &ws, const void *d_jac, size_t n, void *d_out) {
        if (n == 0) return GMSM_OK;
        int rc;
        if ((rc = ws.buckets.ensure(n * sizeof(XYZZL<U>)))) return rc;
        hipLaunchKernelGGL((k_jac_to_recs<U, INLINE_OPS>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ws.stream, d_jac, n,
                           ws.buckets.ptr);
        HIP_TRY(hipGetLastError());
        return normalize_records(ws, n, d_out);
    }

    // ToLagrangeG1 (gmsm_group_fft.h): n = 2^log2n points at d_in - Go-layout affine, or the packed lazy form of registered
    // bases (`packed`) - to d_out, Go-layout affine; d_out may be d_in. Scratch: ws.lagrange (records, the GLV walk's table,
    // the twiddles), ws.buckets (the bit-reversed records), ws.partials (the normalisation's prefix products).
    static constexpr bool LAGRANGE_GLV = GMSM_LAGRANGE_GLV != 0;
    static int to_lagrange(Workspace &ws, const void *d_in, bool packed, unsigned log2n, void *d_out) {
        static_assert(std::is_same<U, FpU<typename LzTraits<U>::Params>>::value, "ToLagrangeG1: coordinates in Fp");
        using Tw = WalkScalar<FrP, LAGRANGE_GLV>;
        using Fld = FftField<FrP>;
        using Fr = Fp<FrP>;
        constexpr size_t REC = sizeof(XYZZL<U>);
        const size_t n = (size_t)1 << log2n, half = n / 2;
        const size_t tab_recs = LAGRANGE_GLV ? 3 * n : 0;  // 3 slots per thread of the widest stage (stage 0: n)
        const size_t tw_off = (n + tab_recs) * REC;
        int rc;
        if ((rc = ws.lagrange.ensure(tw_off + (n + 1) * sizeof(Tw)))) return rc;
        if ((rc = ws.buckets.ensure(n * REC))) return rc;
        char *recs = (char *)ws.lagrange.ptr, *tab = recs + n * REC;
        Tw *tw = (Tw *)(recs + tw_off);
        // buffers: stage 0 runs out of place, the later stages in place, the last one into ws.buckets (the normalisation's
        // input). n = 1: the load alone; n = 2: recs -> buckets; else buckets -> recs -> ... -> recs -> buckets.
        void *const buckets = ws.buckets.ptr;
        void *loaded = log2n == 1 ? (void *)recs : buckets;
        if (packed)
            hipLaunchKernelGGL((k_group_fft_load<U, true>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ws.stream, d_in, n, loaded);
        else
            hipLaunchKernelGGL((k_group_fft_load<U, false>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ws.stream, d_in, n, loaded);
        if (log2n) {
            // w = fr.Generator(n) (as FftField::domain_new), twiddles of w^-1 (computeTwiddlesInv), 1/n
            const Fr w = Fld::pow2k(Fld::from_words(FrP::ROOT_OF_UNITY), FrP::MAX_ORDER - log2n);
            Fr card = Fr::one();
            for (unsigned i = 0; i < log2n; ++i) card = fp_dbl(card);
            hipLaunchKernelGGL((k_group_fft_twiddles<FrP, LAGRANGE_GLV>), dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, ws.stream,
                               Fld::powers_of(fp_inv(w)), fp_inv(card), half, tw);
            for (unsigned s = 0; s < log2n; ++s) {
                const void *src = s == 0 ? loaded : (const void *)recs;
                void *dst = s + 1 == log2n ? buckets : (void *)recs;
                hipLaunchKernelGGL((k_group_fft_stage<typename LzTraits<U>::Params, Consts, FrP, LAGRANGE_GLV, INLINE_OPS>),
                                   dim3((unsigned)(((s ? half : n) + 255) / 256)), dim3(256), 0, ws.stream, src, dst, log2n, s,
                                   (const Tw *)tw, (void *)tab);
            }
        }
        HIP_TRY(hipGetLastError());
        return normalize_records(ws, n, d_out);
    }

    // Variable-base batch (gmsm_scale.h): d_out[i] = s_i d_in[i] for n Go-layout affine points on the device, s_i =
    // d_scalars[i] (Montgomery fr.Elements), d_scalars[0] (`uniform`) or r^i (`r` given, d_scalars unused). d_out may be d_in:
    // every point is a record in ws.buckets before the normalisation writes. Scratch: ws.buckets (the records), ws.lagrange
    // (the walk's table for one chunk of lanes), ws.partials (the normalisation's prefix products).
#ifndef GMSM_SCALE_GLV
#define GMSM_SCALE_GLV 1
#endif
    static constexpr bool SCALE_GLV = GMSM_SCALE_GLV != 0;
    static int batch_scale(Workspace &ws, const void *d_in, size_t n, const void *d_scalars, bool uniform, const Fp<FrP> *r, void *d_out) {
        if (n == 0) return GMSM_OK;
        using Fr = Fp<FrP>;
        constexpr size_t REC = sizeof(XYZZL<U>);
        int rc;
        if ((rc = ws.buckets.ensure(n * REC))) return rc;
        if (SCALE_GLV && (rc = ws.lagrange.ensure(3 * std::min(n, SCALE_CHUNK) * REC))) return rc;
        for (size_t first = 0; first < n; first += SCALE_CHUNK) {
            const size_t count = std::min(SCALE_CHUNK, n - first);
            const dim3 grid((unsigned)((count + 255) / 256)), block(256);
            if (r)
                hipLaunchKernelGGL((k_scale_powers<U, Consts, FrP, SCALE_GLV, INLINE_OPS>), grid, block, 0, ws.stream, d_in, first, count,
                                   FftField<FrP>::powers_of(*r), ws.buckets.ptr, ws.lagrange.ptr);
            else if (uniform)
                hipLaunchKernelGGL((k_batch_scale<U, Consts, FrP, SCALE_GLV, INLINE_OPS, true>), grid, block, 0, ws.stream, d_in, first,
                                   count, (const Fr *)d_scalars, ws.buckets.ptr, ws.lagrange.ptr);
            else
                hipLaunchKernelGGL((k_batch_scale<U, Consts, FrP, SCALE_GLV, INLINE_OPS, false>), grid, block, 0, ws.stream, d_in, first,
                                   count, (const Fr *)d_scalars, ws.buckets.ptr, ws.lagrange.ptr);
        }
        HIP_TRY(hipGetLastError());
        return normalize_records(ws, n, d_out);
    }

    // linearCombinationsG1/G2 (mpcsetup.go:396-447): with powers[i] = r^i and zeros at ends[j] - 1, truncated = MultiExp(A,
    // powers) and shifted = MultiExp(A[1:], powers[:n - 1]) through the device path. n >= 2 and the ends are checked by the
    // caller; `ends` is host memory. Scratch beside the MultiExp's own: ws.poly (the powers, the ends).
    static int linear_combinations(Context &ctx, Workspace &ws, const void *d_points, size_t n, const size_t *ends, size_t n_ends,
                                   const Fp<FrP> &r, J *truncated, J *shifted) {
        using Fr = Fp<FrP>;
        static_assert(sizeof(size_t) == sizeof(uint64_t), "ends are copied as 64-bit words");
        int rc;
        if ((rc = ws.poly.ensure(n * sizeof(Fr) + n_ends * sizeof(uint64_t)))) return rc;
        Fr *pow = (Fr *)ws.poly.ptr;
        uint64_t *d_ends = (uint64_t *)(pow + n);
        HIP_TRY(hipMemcpyAsync(d_ends, ends, n_ends * sizeof(uint64_t), hipMemcpyHostToDevice, ws.stream));
        hipLaunchKernelGGL((k_fft_pow_table<FrP>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ws.stream, FftField<FrP>::powers_of(r),
                           Fr::one(), n, pow, 0u);
        hipLaunchKernelGGL((k_zero_at<FrP>), dim3((unsigned)((n_ends + 255) / 256)), dim3(256), 0, ws.stream, pow, (const uint64_t *)d_ends,
                           n_ends);
        HIP_TRY(hipGetLastError());
        if ((rc = multiexp_device(ctx, ws, d_points, pow, n, ws.stream, truncated, nullptr))) return rc;
        return multiexp_device(ctx, ws, (const char *)d_points + AFF_BYTES, pow, n - 1, ws.stream, shifted, nullptr);
    }

    // Rewrites n Go-layout bases (device memory) into the lazy domain once; the result serves any number of MultiExp
    // calls over a prefix of the bases (kzg.Commit over pk.G1[:len(p)], ecc/bn254/kzg/kzg.go:159-176).
    static int register_bases(Context &ctx, const void *d_points, size_t n, hipStream_t stream, ResidentBases *out) {
        int rc;
        if ((rc = out->upoints.ensure(n * AFF_BYTES))) return rc;
        if ((rc = out->skip.ensure(n))) return rc;
        if (n) {
            hipLaunchKernelGGL((k_convert_points<U>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_points, n,
                               out->upoints.ptr, (uint8_t *)out->skip.ptr);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipStreamSynchronize(stream));
        }
        out->n = n;
        return GMSM_OK;
    }

    // ---- N4: point ingest (gmsm_ingest.h). Results of the checks come back through one 64-bit word:
    // (index << 3 | PointStatus) of the first offending point, all ones when every point passed.
    static int read_first_bad(Workspace &ws, long long *bad_index, uint32_t *status) {
        unsigned long long v = 0;
        HIP_TRY(hipMemcpyAsync(&v, ws.flagword.ptr, 8, hipMemcpyDeviceToHost, ws.stream));
        HIP_TRY(hipStreamSynchronize(ws.stream));
        if (v == ~0ull) {
            *bad_index = -1;
            *status = PT_OK;
        } else {
            *bad_index = (long long)(v >> 3);
            *status = (uint32_t)(v & 7u);
        }
        return GMSM_OK;
    }
    // d_raw: n wire-format points on the device -> d_out: n Go-layout affine points (Montgomery)
    static int decode_raw(Workspace &ws, const void *d_raw, size_t n, int level, void *d_out, long long *bad_index,
                          uint32_t *status) {
        int rc;
        if ((rc = ws.flagword.ensure(8))) return rc;
        HIP_TRY(hipMemsetAsync(ws.flagword.ptr, 0xff, 8, ws.stream));
        if (n)
        {
            const dim3 grid((unsigned)((n + 127) / 128));
            if (level >= 3 && NEEDS_TORSION)
                hipLaunchKernelGGL((k_decode_raw<F, FrP, Consts, NEEDS_TORSION, NEEDS_TORSION>), grid, dim3(128), 0, ws.stream,
                                   (const uint8_t *)d_raw, n, level, (Aff *)d_out, (unsigned long long *)ws.flagword.ptr);
            else
                hipLaunchKernelGGL((k_decode_raw<F, FrP, Consts, NEEDS_TORSION, false>), grid, dim3(128), 0, ws.stream,
                                   (const uint8_t *)d_raw, n, level, (Aff *)d_out, (unsigned long long *)ws.flagword.ptr);
        }
        HIP_TRY(hipGetLastError());
        return read_first_bad(ws, bad_index, status);
    }
    // d_comp: n compressed points (Bytes(), sizeof(F) bytes each) -> d_out: n Go-layout affine points; level >= 2 adds the
    // subgroup check of the decoded points (the Decoder's default, marshal.go:300-330): a second launch, and the smaller
    // index of the two kinds of offender is the one reported (the reference stops at the first error of either kind).
    static int decode_compressed(Workspace &ws, const void *d_comp, size_t n, int level, void *d_out, long long *bad_index,
                                 uint32_t *status) {
        int rc;
        if ((rc = ws.flagword.ensure(8))) return rc;
        HIP_TRY(hipMemsetAsync(ws.flagword.ptr, 0xff, 8, ws.stream));
        if (n) {
            hipLaunchKernelGGL((k_decompress<F, Consts>), dim3((unsigned)((n + 127) / 128)), dim3(128), 0, ws.stream,
                               (const uint8_t *)d_comp, n, (Aff *)d_out, (unsigned long long *)ws.flagword.ptr);
            // offenders were written as infinity, which passes: the word keeps the decoder's verdict for them
            if (level >= 2 && NEEDS_TORSION) launch_validate(ws, d_out, n, level);
        }
        HIP_TRY(hipGetLastError());
        return read_first_bad(ws, bad_index, status);
    }
    // (*G1Affine).Bytes over a vector: d_points -> d_comp (n * sizeof(F) bytes)
    static int encode_compressed(Workspace &ws, const void *d_points, size_t n, void *d_comp) {
        if (n)
            hipLaunchKernelGGL((k_compress<F, Consts>), dim3((unsigned)((n + 127) / 128)), dim3(128), 0, ws.stream,
                               (const Aff *)d_points, n, (uint8_t *)d_comp);
        HIP_TRY(hipGetLastError());
        return GMSM_OK;
    }
    static void launch_validate(Workspace &ws, const void *d_points, size_t n, int level) {
        const dim3 grid((unsigned)((n + 127) / 128));
        if (level >= 3 && NEEDS_TORSION)  // the definition [r]P = infinity: its own kernel (gmsm_ingest.h, BY_DEF)
            hipLaunchKernelGGL((k_validate_points<F, FrP, Consts, NEEDS_TORSION, NEEDS_TORSION>), grid, dim3(128), 0, ws.stream,
                               (const Aff *)d_points, n, level, (unsigned long long *)ws.flagword.ptr);
        else
            hipLaunchKernelGGL((k_validate_points<F, FrP, Consts, NEEDS_TORSION, false>), grid, dim3(128), 0, ws.stream,
                               (const Aff *)d_points, n, level, (unsigned long long *)ws.flagword.ptr);
    }
    static int validate_points(Workspace &ws, const void *d_points, size_t n, int level, long long *bad_index,
                               uint32_t *status) {
        int rc;
        if ((rc = ws.flagword.ensure(8))) return rc;
        HIP_TRY(hipMemsetAsync(ws.flagword.ptr, 0xff, 8, ws.stream));
        if (n && level > 0) launch_validate(ws, d_points, n, level);
        HIP_TRY(hipGetLastError());
        return read_first_bad(ws, bad_index, status);
    }

    // Most points one pipeline run takes: the coarse partition pass keeps two 32-bit words per partition in LDS, which
    // caps it at 2^27 references per window. Larger inputs run as consecutive point ranges whose window totals are added
    // (the point decomposition of sharding.py, on one device). GMSM_OPT_MAX_RUN lowers the cap (tests).
    // A shared-bucket plan (window tables) sorts nwin * n entries as one window: a sort entry is 32 bits - the low
    // bucket bits of the coarse pass next to (index, sign) - and the coarse pass takes at most 2^13 partitions.
    static size_t max_run_points(const WindowPlan &plan = WindowPlan{0, 0, 0, 0, 1, 0, 0, 0}) {
        size_t cap = (size_t)1 << 27;
        if (plan.glv) cap >>= 1;  // two entries per point
        if (plan.shared) {
            uint32_t log2NB = 0;
            while ((1u << log2NB) < plan.nbuckets) ++log2NB;
            const uint32_t fb_min = log2NB > 13 ? log2NB - 13 : 0;
            cap = std::min(cap, (((size_t)1 << (31 - fb_min)) - 1) / plan.nwin_total);
        }
        const size_t forced = options().max_run.load(std::memory_order_relaxed);
        return forced ? std::min(cap, forced) : cap;
    }

    // ---- window tables of registered bases (gmsm_bases_precompute): table slab w = 2^(c w) P_i for every window w of the
    // c-bit decomposition, so that the digits of ALL windows index one bucket set - one reduction of 2^(c-1) buckets
    // instead of nwin of them, which in turn lets c grow (fewer windows = fewer additions). 288 GB of HBM pay for it:
    // nwin copies of the bases (BN254 G1, 2^20 points, c = 19: 14 x 64 MiB).
    // GMSM_OPT_TABLES: 0 = never, 1 (default) = the measured range of call sizes, 2 = whenever the handle has tables (tests)
    static bool tables_serve(size_t n_registered, size_t n_call) {
        const unsigned mode = options().tables.load(std::memory_order_relaxed);
        if (mode == 0 || n_call == 0) return false;
        if (mode >= 2) return true;
        if (n_call < table_min_points() || n_call > table_max_points()) return false;
        return n_call * 16 >= n_registered;  // a short prefix of the bases: the tables' window is too wide for it
    }
    static bool use_tables(const ResidentBases *rb, size_t n) {
        if (!rb || rb->tab_c.load() == 0) return false;
        const unsigned forced = options().window_bits.load(std::memory_order_relaxed);
        if (forced >= 2 && forced <= 20 && forced != rb->tab_c.load()) return false;
        return tables_serve(rb->n, n);
    }
    // The plan of a MultiExp over n points: the measured window table, or the registered bases' tables when they exist
    static WindowPlan plan_for(const ResidentBases *rb, size_t n) {
        if (use_tables(rb, n)) {
            WindowPlan plan = make_plan(rb->tab_c.load(), 0, 1);
            plan.shared = 1;
            return plan;
        }
        if (rb == nullptr) {  // bases taken anew: GLV half scalars where they were measured ahead (glv_preferred_c)
            const unsigned mode = options().glv.load(std::memory_order_relaxed);
            const unsigned forced = options().window_bits.load(std::memory_order_relaxed);
            unsigned c = 0;
            if (mode >= 2) c = choose_c(FR_BITS, AFF_BYTES, 2 * n);           // always (A/B): the width of a 2 n-point call, or the forced one
            else if (mode == 1 && forced == 0) c = glv_preferred_c(FR_BITS, AFF_BYTES, n);
            if (c != 0 && glv_width_built(c)) return make_plan_glv(c, 0, 1);
        }
        return make_plan(choose_c(FR_BITS, AFF_BYTES, n), 0, 1);
    }
    // Default table width for n registered points, from sweeps of every group over 2^13..2^21 with the width forced
    // (tools/tables_sweep.py, profiles/r03_tables.log). What moves it away from the plain path's width: the shared set
    // holds nwin * n entries, so (a) a wider window pays twice - fewer slabs to add AND shorter chains of partial sums
    // per bucket (nwin n / 2^(c-1) entries per bucket; BW6-761 2^18: fix-up 1.83 ms at c = 14, 0.10 ms at c = 18) -,
    // (b) one reduction of 2^(c-1) buckets is cheap next to nwin of them, and (c) the TOP window must not be narrow: a
    // top window of t bits drops its n entries into 2^t buckets of the one set (BN254 at c = 19: 7 bits, a million
    // entries in 128 buckets, i.e. in one coarse partition - 0.9 ms of fine sort), which rules out 18, 19 for BN254,
    // 17, 18 for BLS12-381 (17 also fills the top window: the carry doubles the buckets) and 15..17 for BW6-761.
    static unsigned table_c(size_t n) {
        unsigned lg = 0;
        while (((size_t)2 << lg) <= n) ++lg;
        if (FR_BITS > 300) return 18;                                        // BW6-761
        if (AFF_BYTES == 64) return lg <= 14 ? 15 : lg <= 18 ? 16 : 17;      // BN254 G1
        if (FR_BITS == 254) return lg <= 16 ? 15 : lg <= 19 ? 16 : 20;       // BN254 G2
        return lg < 20 ? 16 : 20;                                            // BLS12-381 G1, G2
    }
    // Call sizes the tables serve (measured against the plain path, same sweeps): below, a call is all latency and the
    // plain path's narrow windows win; above, the one window of nwin * n entries costs more in the sort and in the chains
    // of partial sums than one reduction saves (BN254 G1 2^22: 6.02 against 5.90 ms), and wider tables would need sort
    // entries of more than 32 bits.
    static size_t table_min_points() { return (size_t)1 << (AFF_BYTES == 64 ? 13 : 15); }
    static size_t table_max_points() { return (size_t)3 << (FR_BITS == 255 && AFF_BYTES == 96 ? 19 : 20); }
    // slabs 1 .. nw-1 of a table over the first m registered bases (slab 0 = the bases themselves, copied): slab w = slab
    // w-1 doubled c times. `bad` != 0 afterwards: a multiple of a base reached the identity.
    static int build_table_slabs(Workspace &ws, const ResidentBases *rb, size_t m, unsigned c, uint32_t nw, void *tables, uint32_t *bad) {
        const size_t slab = m * AFF_BYTES;
        int rc;
        if ((rc = ws.buckets.ensure(m * sizeof(XYZZL<U>)))) return rc;
        if ((rc = ws.h2d_points.ensure(slab))) return rc;
        if ((rc = ws.skip.ensure(m))) return rc;
        if ((rc = ws.flagword.ensure(8))) return rc;
        HIP_TRY(hipMemsetAsync(ws.flagword.ptr, 0, 8, ws.stream));
        HIP_TRY(hipMemcpyAsync(tables, rb->upoints.ptr, slab, hipMemcpyDeviceToDevice, ws.stream));
        const dim3 grid((unsigned)((m + 255) / 256)), block(256);
        for (uint32_t w = 1; w < nw; ++w) {
            char *prev = (char *)tables + (size_t)(w - 1) * slab;
            hipLaunchKernelGGL((k_table_double<U, INLINE_OPS>), grid, block, 0, ws.stream, (const void *)prev,
                               (const uint8_t *)rb->skip.ptr, m, c, ws.buckets.ptr);
            if ((rc = normalize_records(ws, m, ws.h2d_points.ptr))) return rc;
            hipLaunchKernelGGL((k_convert_points<U>), grid, block, 0, ws.stream, (const void *)ws.h2d_points.ptr, m,
                               (void *)(prev + slab), (uint8_t *)ws.skip.ptr);
            hipLaunchKernelGGL(k_skip_mismatch, grid, block, 0, ws.stream, (const uint8_t *)rb->skip.ptr,
                               (const uint8_t *)ws.skip.ptr, m, (uint32_t *)ws.flagword.ptr);
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(bad, ws.flagword.ptr, 4, hipMemcpyDeviceToHost, ws.stream));
        HIP_TRY(hipStreamSynchronize(ws.stream));
        return GMSM_OK;
    }
    static constexpr unsigned SMALL_TABLE_C = 6;          // width of the narrow tables: 2^5 buckets, one lane quad each
    // ... over the first so many bases (43 x 4096 x 64 B = 11 MiB for BN254 G1). Measured against the other forms (profiles/r05_small_n.log,
    // last block): ahead up to 2^12 points for every group but BW6-761 (2^12: 2.36 ms against 2.08 for the sorted pipeline; 2^10: 0.70 against 1.07)
    static constexpr size_t SMALL_TABLE_POINTS = FR_BITS > 300 ? 2048 : 4096;
    static int precompute_tables(Context &ctx, Workspace &ws, ResidentBases *rb, unsigned c) {
        if (c == 0) c = table_c(rb->n);
        if (c < 2 || c > 20) return fail(GMSM_ERR_ARG, "table window width must be 2..20");
        if (rb->n == 0 || rb->n >= ((size_t)1 << 31)) return fail(GMSM_ERR_ARG, "window tables need 1 <= n < 2^31 bases");
        const WindowPlan plan = make_plan(c, 0, 1);
        const uint32_t nw = plan.nwin_total;
        const size_t n = rb->n, slab = n * AFF_BYTES;
        int rc;
        if ((rc = rb->tables.ensure((size_t)nw * slab))) return rc;
        if ((rc = order_after(ws, nullptr))) return rc;
        uint32_t bad = 0;
        if ((rc = build_table_slabs(ws, rb, n, c, nw, rb->tables.ptr, &bad))) return rc;
        if (bad) {  // a base of even order (not a subgroup point): its multiples reach the identity - no tables, plain path
            rb->tables.release();
            return fail(GMSM_ERR_ARG, "window tables: a multiple 2^k P of a base is the identity (bases outside the prime-order subgroup)");
        }
        rb->tab_nw = nw;
        rb->tab_c.store(c, std::memory_order_release);  // publication: everything above is complete (stream synchronised)
        // the narrow tables of the fused small-n kernel: calls of a few thousand points over these bases then fill ONE
        // bucket set per workgroup and need no host-side fold at all (enqueue_small, shared form)
        {
            const WindowPlan sp = make_plan(SMALL_TABLE_C, 0, 1);
            const size_t m = std::min<size_t>(n, SMALL_TABLE_POINTS);
            if (rb->small_tables.ensure((size_t)sp.nwin_total * m * AFF_BYTES) == GMSM_OK &&
                build_table_slabs(ws, rb, m, SMALL_TABLE_C, sp.nwin_total, rb->small_tables.ptr, &bad) == GMSM_OK && !bad) {
                rb->small_nw = sp.nwin_total;
                rb->small_m = m;
                rb->small_c.store(SMALL_TABLE_C, std::memory_order_release);
            } else {
                // the narrow tables are an extra: without them small calls over the handle take the plain fused kernel. Their
                // memory goes back and the failure's text does not linger as this thread's last error (the call succeeded).
                rb->small_tables.release();
                clear_last_error();
            }
        }
        return GMSM_OK;
    }

    // Point ranges of a MultiExp over device-resident inputs. More than one range (a) beyond the cap of one pipeline run
    // and (b) - experiment, GMSM_DEVICE_RANGES - to keep the bases of a range inside the 256 MiB Infinity Cache while
    // all windows gather from them.
    static unsigned device_ranges(size_t n, const WindowPlan &plan) {
        size_t run = max_run_points(plan);
        // BN254 G1 beyond 2^24 points: ranges of 2^24. The coarse sort of a longer run has 2048+ partitions and writes
        // 8-entry runs (scatter + fine sort 4.2 ms at 2^25, 9.0 at 2^26, against 1.45 per 2^24 points); the ranges share one
        // bucket set and one reduction, a merge costs 0.1 ms: 2^25 43.8 -> 42.0 ms, 2^26 86.3 -> 83.0 (profiles/r05_device_ranges.log).
        // Neutral for BLS12-381 G1 (84.6 / 84.4-84.7 ms at 2^25) and worse below 2^24 (BN254 G1 2^24 in two ranges: 21.5 -> 22.0).
        if (AFF_BYTES == 64 && !plan.shared && options().max_run.load(std::memory_order_relaxed) == 0) run = std::min<size_t>(run, (size_t)1 << 24);
        unsigned nr = (unsigned)((n + run - 1) / run);
        const unsigned forced = GMSM_TUNE(DEVICE_RANGES, 0);
        if (forced > nr) nr = (unsigned)std::min<size_t>(forced, n);
        return nr;
    }

    // ---- the fused small-n kernel (gmsm_small.h): calls of at most small_max_points() points that neither force a window
    // width nor are served by window tables. The width minimises the depth of the kernel's dependency chain -
    // log2(points per bucket) + 2 (c - 1) additions - against the number of windows the host has to fold.
    static constexpr uint32_t SMALL_SL = SmallSlice<U>::value;
    static constexpr bool SMALL_QUAD_ONLY = SmallQuadOnly<U>::value;
    // Measured against the sorted pipeline (profiles/r05_small_n.log, resident ms, fused / pipeline): BN254 G1 2^5 0.147 / 0.27,
    // 2^10 0.18 / 0.29-0.35, 2^12 0.28 / 0.41, 2^13 0.38 / 0.47; BN254 G2 2^11 0.65 / 0.91, 2^13 1.29 / 0.99; BLS12-381 G1 2^11 0.41 /
    // 0.62, 2^12 0.50 / 0.65, 2^13 0.73 / 0.70; BLS12-381 G2 2^11 1.19 / 1.62, 2^12 1.68 / 1.65; BN254 G2 2^12 0.86 / 0.86; BW6-761 2^11 1.57 / 2.05,
    // 2^12 2.5 / 2.1. Round 6 (GLV half scalars, lane quads for the bucket phase): profiles/r06_small_n.log.
    // Largest call the fused kernel takes, from the same-process sweeps of profiles/r06_small_forms.log (fused / sorted pipeline,
    // resident ms): BN254 G1 2^13 0.36 / 0.46; BLS12-381 G1 2^12 0.47 / 0.65, 2^13 0.69 / 0.69; BN254 G2 2^12 0.83 / 0.88, 2^13
    // 1.12 / 0.90; BLS12-381 G2 2^10 0.98 / 1.87, 2^11 1.60-1.68 / 1.63; BW6-761 2^10 1.61 / 2.41, 2^11 2.73 / 2.07 (the quad form
    // keeps one workgroup per CU at 310 registers: beyond ~1000 points the wide types are throughput-bound there).
    static size_t small_max_points() {
        const size_t forced = options().small_max.load(std::memory_order_relaxed);
        return std::min<size_t>(forced ? forced : GMSM_TUNE(SMALL_MAX, sizeof(U) <= 36 ? 8192 : sizeof(U) <= 72 ? 4096 : 1024),
                                small_entry_cap() / 2);
    }
    // entries one window's slices can hold: 64 slices of 256 entries (one-lane form) or of 8 chunks of 64 (quad form)
    static constexpr size_t small_entry_cap() {
        return SMALL_QUAD_ONLY ? (size_t)SMALL_QUAD_ENTRIES * SMALL_QUAD_MAX_CHUNKS * SMALL_MAX_SLICES : (size_t)SMALL_SL * SMALL_MAX_SLICES;
    }
    // GLV half scalars in the fused kernel: unless GMSM_OPT_GLV = 0
    static bool small_glv() { return options().glv.load(std::memory_order_relaxed) >= 1; }
    static WindowPlan small_make_plan(unsigned c, bool glv) { return glv ? make_plan_glv(c, 0, 1) : make_plan(c, 0, 1); }
    static unsigned small_c(size_t n, bool glv) {
        const unsigned forced = options().small_bits.load(std::memory_order_relaxed);
        // flat over 5..7 for the narrow types (fewer windows = less host fold, more buckets = more quad steps); the 28-limb
        // field and large calls take 7
        const size_t entries = glv ? 2 * n : n;
        unsigned c = (forced >= 2 && forced <= SMALL_MAX_C) ? forced
                     : FR_BITS > 300 ? (entries <= 512 ? 6 : 7)
                                     : entries <= 256 ? 5 : entries <= 4096 ? 6 : 7;
        // the kernel holds one lane quad per bucket: a width whose top window needs c + 1 bits (the scalar's bit
        // length a multiple of c) doubles the buckets - step down until they fit
        while (c > 2 && small_make_plan(c, glv).nbuckets > SMALL_NB_MAX) --c;
        return c;
    }
    static bool small_serves(size_t n, const ResidentBases *rb) {
        if (options().small_bits.load(std::memory_order_relaxed) == 1) return false;
        if (options().window_bits.load(std::memory_order_relaxed) != 0) return false;  // a forced width: the sorted pipeline
        if (small_shared(n, rb)) return true;
        return n >= 1 && n <= small_max_points() && !use_tables(rb, n);
    }
    // the narrow window tables of registered bases serve the call: every (window, point) pair is an entry of ONE bucket set
    static bool small_shared(size_t n, const ResidentBases *rb) {
        if (!rb || n < 1 || options().tables.load(std::memory_order_relaxed) == 0) return false;
        const unsigned c = rb->small_c.load(std::memory_order_acquire);
        if (c == 0 || n > rb->small_m) return false;
        const unsigned forced = options().small_bits.load(std::memory_order_relaxed);
        if (forced >= 2 && forced != c) return false;
        return n * rb->small_nw <= (size_t)SMALL_SL * SMALL_SHARED_MAX_SLICES;
    }
    // What one call of the fused kernel looks like; decided ONCE per call (options and the publication of the narrow tables
    // are read here and nowhere else on the call's path).
    struct SmallPlan {
        WindowPlan plan;
        bool shared, glv, quad;
        uint32_t chunks, nslices;
    };
    static SmallPlan small_plan(size_t n, const ResidentBases *rb) {
        SmallPlan sp;
        sp.shared = small_shared(n, rb);
        sp.glv = !sp.shared && small_glv();
        sp.plan = sp.shared ? make_plan(rb->small_c.load(), 0, 1) : small_make_plan(small_c(n, sp.glv), sp.glv);
        const size_t entries = sp.shared ? n * sp.plan.nwin_total : (sp.glv ? 2 * n : n);
        // the bucket phase on lane quads (64 entries per chunk): always for the wide element types; for the narrow ones while
        // the call is so small that a workgroup per 64 entries still leaves CUs idle (GMSM_OPT_SMALL_QUAD: 0 = this rule,
        // 1 = never, 2 = always)
        const unsigned fq = options().small_quad.load(std::memory_order_relaxed);
        const size_t wgs64 = (entries + SMALL_QUAD_ENTRIES - 1) / SMALL_QUAD_ENTRIES * (sp.shared ? 1 : sp.plan.nwin_total);
        sp.quad = SMALL_QUAD_ONLY || fq == 2 || (fq == 0 && wgs64 <= (size_t)GMSM_TUNE(SMALL_QUAD_WGS, 512));
        if (sp.quad) {
            const size_t max_slices = sp.shared ? SMALL_SHARED_MAX_SLICES : SMALL_MAX_SLICES;
            size_t chunks = 1;
            while ((entries + chunks * SMALL_QUAD_ENTRIES - 1) / (chunks * SMALL_QUAD_ENTRIES) > max_slices) chunks *= 2;
            // every workgroup ends with the same 2 (c - 1) + log2(slices) reduction steps whatever it accumulated: once the
            // launch has more workgroups than the chip holds at a time (one per CU for the wide types: 310 registers, 89 KB of
            // LDS), longer walks per workgroup beat more workgroups (BW6-761 2^10: 896 workgroups of one chunk 1.61 ms)
            const size_t nsets = sp.shared ? 1 : sp.plan.nwin_total, resident_wgs = SMALL_QUAD_ONLY ? 256 : 768;
            while (chunks < SMALL_QUAD_MAX_CHUNKS &&
                   (entries + chunks * SMALL_QUAD_ENTRIES - 1) / (chunks * SMALL_QUAD_ENTRIES) * nsets > resident_wgs &&
                   entries > chunks * SMALL_QUAD_ENTRIES)
                chunks *= 2;
            sp.chunks = (uint32_t)chunks;
            sp.nslices = (uint32_t)((entries + chunks * SMALL_QUAD_ENTRIES - 1) / (chunks * SMALL_QUAD_ENTRIES));
        } else {
            sp.chunks = 0;
            sp.nslices = (uint32_t)((entries + SMALL_SL - 1) / SMALL_SL);
        }
        return sp;
    }
    // Enqueues the kernel on ws.stream; the window totals (shared form: ONE total) land in ws.pinned. d_points == nullptr:
    // `resident`.
    static int enqueue_small(Context &ctx, Workspace &ws, const void *d_points, const void *d_scalars, size_t n,
                             const SmallPlan &sp, const ResidentBases *resident) {
        const WindowPlan &plan = sp.plan;
        const uint32_t nw = sp.shared ? 1u : plan.nwin_total;
        constexpr size_t REC = sizeof(typename OpsSerial::Mem);
        int rc;
        ws.pending_timed = false;
        ws.plane_np = 0;
        if ((rc = begin_use(ws, ws.stream))) return rc;
        if ((rc = ws.ensure_pinned((size_t)plan.nwin_total * sizeof(Ext)))) return rc;
        if ((rc = ws.small_sums.ensure((size_t)nw * sp.nslices * REC))) return rc;
        if ((rc = ws.small_done.ensure((size_t)HEAVY_MAX_WINDOWS * 4))) return rc;
        // the slice counters start at zero: cleared before every launch that uses them (a launch that died half-way must not
        // leave a later call without its last workgroup - advisor, round 5)
        if (sp.nslices > 1) HIP_TRY(hipMemsetAsync(ws.small_done.ptr, 0, (size_t)nw * 4, ws.stream));
        SmallArgs a;
        a.points = d_points;
        a.upoints = nullptr;
        a.skip = nullptr;
        if (d_points == nullptr) {
            a.upoints = sp.shared ? resident->small_tables.ptr : resident->upoints.ptr;
            a.skip = (const uint8_t *)resident->skip.ptr;
        }
        a.scalars = (const uint32_t *)d_scalars;
        a.n = (uint32_t)n;
        a.glv = sp.glv ? 1u : 0u;
        a.tab_m = sp.shared ? (uint32_t)resident->small_m : 0u;
        a.chunks = sp.chunks;
        a.slice_sums = ws.small_sums.ptr;
        a.done = (uint32_t *)ws.small_done.ptr;
        // the window totals go straight into the pinned result buffer (host memory mapped into the device: nwin 128-byte
        // stores over PCIe instead of a copy kernel and its launch, 5-8 us of a 0.15 ms call)
        a.totals = ws.pinned;
        g_small_runs.fetch_add(1, std::memory_order_relaxed);
        if (sp.shared) g_table_runs.fetch_add(1, std::memory_order_relaxed);
        // profiling: the one launch counts as the call's accumulation stage (two events, whatever the level)
        StageTimer timer(ws, true);
        ws.timed = timer.on;
        if (timer.on) {
            ws.timed_level = 2;
            (void)hipEventRecord(ws.events[T_ACCUMULATE], ws.stream);
        }
        const dim3 grid(sp.nslices, nw);
        if (sp.quad) {
            const size_t lds = (size_t)192 * sizeof(QRec<U>);
            if (sp.shared) {
                if ((rc = ctx.allow_lds((const void *)k_msm_small_q<U, FrP, Consts, true>, (int)lds))) return rc;
                hipLaunchKernelGGL((k_msm_small_q<U, FrP, Consts, true>), grid, dim3(256), lds, ws.stream, a, plan);
            } else {
                if ((rc = ctx.allow_lds((const void *)k_msm_small_q<U, FrP, Consts, false>, (int)lds))) return rc;
                hipLaunchKernelGGL((k_msm_small_q<U, FrP, Consts, false>), grid, dim3(256), lds, ws.stream, a, plan);
            }
        } else {
            if constexpr (!SMALL_QUAD_ONLY) {
                const size_t lds = (size_t)SMALL_SL * REC;
                if (sp.shared) {
                    if ((rc = ctx.allow_lds((const void *)k_msm_small<U, FrP, Consts, SMALL_SL, true>, (int)lds))) return rc;
                    hipLaunchKernelGGL((k_msm_small<U, FrP, Consts, SMALL_SL, true>), grid, dim3(SMALL_SL), lds, ws.stream, a, plan);
                } else {
                    if ((rc = ctx.allow_lds((const void *)k_msm_small<U, FrP, Consts, SMALL_SL, false>, (int)lds))) return rc;
                    hipLaunchKernelGGL((k_msm_small<U, FrP, Consts, SMALL_SL, false>), grid, dim3(SMALL_SL), lds, ws.stream, a, plan);
                }
            }
        }
        HIP_TRY(hipGetLastError());
        if (timer.on) (void)hipEventRecord(ws.events[T_FIXUP], ws.stream);
        ws.pending_timed = timer.on;
        return end_use(ws, ws.stream);
    }
    // waits for an enqueue_small and turns what it left in ws.pinned into the result
    static int collect_small(Workspace &ws, const SmallPlan &sp, J *out) {
        if (sp.shared) {  // one total, nothing to fold
            Ext total;
            int rc = collect_window_sums(ws, ws.stream, 1, &total);
            if (rc) return rc;
            *out = total.zz.is_zero() ? J{F::one(), F::one(), F::zero()} : jac_from_xyzz(total);
            return GMSM_OK;
        }
        std::vector<Ext> totals(sp.plan.nwin_total);
        int rc = collect_window_sums(ws, ws.stream, sp.plan.nwin_total, totals.data());
        if (rc) return rc;
        *out = fold(totals.data(), sp.plan.c, sp.plan.nwin_total);
        return GMSM_OK;
    }
    static int multiexp_small(Context &ctx, Workspace &ws, const void *d_points, const void *d_scalars, size_t n,
                              hipStream_t caller_stream, J *out, const ResidentBases *resident) {
        const SmallPlan sp = small_plan(n, d_points ? nullptr : resident);
        if (sp.plan.nwin_total > HEAVY_MAX_WINDOWS) return fail(GMSM_ERR_ARG, "small path: too many windows");
        int rc = order_after(ws, caller_stream);
        if (rc) return rc;
        if ((rc = enqueue_small(ctx, ws, d_points, d_scalars, n, sp, resident))) return rc;
        return collect_small(ws, sp, out);
    }

    static int multiexp_device(Context &ctx, Workspace &ws, const void *d_points, const void *d_scalars, size_t n,
                               hipStream_t caller_stream, J *out, const ResidentBases *resident = nullptr) {
        if (small_serves(n, resident)) return multiexp_small(ctx, ws, d_points, d_scalars, n, caller_stream, out, resident);
        const WindowPlan plan = plan_for(resident, n);
        const unsigned c = plan.c;
        const unsigned nr = device_ranges(n, plan);
        if (nr <= 1) return window_sums_folded(ctx, ws, d_points, d_scalars, n, plan, caller_stream, out, resident);
        std::vector<Ext> totals(plan.nwin_total);
        // Consecutive point ranges on the workspace's stream: each leaves its bucket sums, k_merge_buckets adds them to the
        // running buckets, one reduction at the end (the reference's split + AddAssign, multiexp.go:98-140, bucket by bucket).
        constexpr size_t REC = sizeof(typename OpsSerial::Mem);
        const size_t per = (n + nr - 1) / nr;
        int rc = order_after(ws, caller_stream);
        if (rc) return rc;
        if ((rc = ws.carry.ensure((size_t)bucket_sets(plan) * plan.nbuckets * REC))) return rc;
        // stage profile of a multi-range call: every range's events are collected before the next range reuses them (one
        // stream synchronisation per range, profiling only), the call counts once; the final reduction is not in it
        const bool prof = profiling_level() != 0;
        float pms[STAGE_COUNT] = {0};
        unsigned plaunch[STAGE_COUNT] = {0};
        for (unsigned r = 0; r * per < n; ++r) {
            const size_t lo = (size_t)r * per, len = std::min(per, n - lo);
            const void *dp = d_points ? (const char *)d_points + lo * AFF_BYTES : nullptr;
            RunRequest rq;
            rq.resident_offset = lo;
            rq.buckets_only = true;
            rq.time_range = prof;
            if ((rc = enqueue_window_sums(ctx, ws, dp, (const char *)d_scalars + lo * SCALAR_BYTES, len, plan, ws.stream, resident, rq)))
                return rc;
            if (prof && ws.pending_timed) {
                HIP_TRY(wait_stream(ws.stream));
                StageTimer::collect_add(ws, pms, plaunch);
                ws.pending_timed = false;
            }
            hipLaunchKernelGGL((k_merge_buckets<OpsSerial>), dim3((plan.nbuckets + 255) / 256, bucket_sets(plan)), dim3(256), 0, ws.stream,
                               ws.carry.ptr, (const void *)ws.buckets.ptr, (const uint32_t *)ws.starts.ptr, plan.nbuckets, r == 0 ? 1 : 0);
        }
        if ((rc = enqueue_reduce(ctx, ws, ws.carry.ptr, plan, per, ws.stream))) return rc;
        if ((rc = collect_window_sums(ws, ws.stream, plan.nwin_local, totals.data()))) return rc;
        if (prof) record_stage_times(pms, plaunch);
        *out = fold(totals.data(), c, plan.nwin_total);
        return GMSM_OK;
    }

    // Asynchronous pair (gmsm_multiexp_bases_submit / gmsm_multiexp_collect): submit launches the whole device pipeline
    // on the workspace's own stream and returns; collect waits for it, then folds the windows on the host.
    static int multiexp_submit(Context &ctx, Workspace &ws, const void *d_scalars, size_t n, const ResidentBases *resident) {
        if (n > max_run_points())
            return fail(GMSM_ERR_ARG, "submit/collect takes at most 2^27 points per ticket: use the blocking entry, which splits larger inputs");
        WindowPlan plan = plan_for(resident, n);
        if (n > max_run_points(plan)) plan = make_plan(choose_c(FR_BITS, AFF_BYTES, n), 0, 1);  // one run per ticket: plain path
        const unsigned c = plan.c;
        RunRequest rq;
        rq.tail_mode = TAIL_AUTO;
        int rc = enqueue_window_sums(ctx, ws, nullptr, d_scalars, n, plan, ws.stream, resident, rq);
        if (rc) return rc;
        ws.pending_c = c;
        ws.pending_nw = plan.nwin_total;
        return GMSM_OK;
    }
    static int multiexp_collect(Workspace &ws, J *out) {
        return collect_folded(ws, ws.stream, ws.pending_c, ws.pending_nw, out);
    }

    // Number of point ranges a host-buffer MultiExp is cut into so that the H2D copy of range k+1 runs under the
    // pipeline of range k (two workspaces, two streams). Round 2 reduced every range on its own and added the totals on
    // the host: a range then paid the size-independent part of the pipeline again (0.35 ms reduction chain), so 2^20 ran
    // as 2 ranges (cold 3.99 / 3.31 / 3.94 ms with 1 / 2 / 4 ranges, profiles/r02_host_ranges.log). Now the ranges share one
    // bucket set and ONE reduction (k_merge_buckets), a range costs its share of the accumulation plus ~0.1 ms, and the
    // call is cut finer: what is exposed is the copy of the first range and the tail after the last.
    // GMSM_OPT_HOST_RANGES overrides.
    static unsigned host_ranges(size_t n, bool with_points) {
        const unsigned forced = options().host_ranges.load(std::memory_order_relaxed);
        if (forced) return (unsigned)std::min<size_t>(forced, std::max<size_t>(1, n));
        // Measured (profiles/r03_host_ranges.log, BN254 G1, cold / warm-bases ms): 2^20 1 range 3.73 / 2.51, 2: 3.19 / 2.23,
        // 4: 2.95 / 2.31, 8: 3.38 / 2.70; 2^22 4: 9.47 / 6.97, 8: 8.87 / 7.11, 16: 9.69 / 8.26; 2^24 8: 32.5 / 23.5, 16: 31.5 / 23.3,
        // 32: 31.8 / 25.1 (resident 2.00 / 6.25 / 22.1): a range costs about 0.1 ms of launches and merge.
        if (with_points) {  // bases + scalars cross PCIe (96 B per BN254 G1 point)
            if (n < ((size_t)1 << 19)) return 1;
            if (n < ((size_t)1 << 23)) return (unsigned)std::min<size_t>(8, n >> 18);
            return 16;
        }
        if (n < ((size_t)1 << 20)) return 1;  // scalars only (32 B per point)
        // the two G1 groups of 64 / 96-byte points: three to eight ranges, the first (and, from four, the last) half as long
        // (window_sums_from_host); the wider groups compute 3-10 times longer per point - the copy hardly shows, every
        // range costs its launches: few, uniform ranges (BN254 G2 2^20: 6.19 ms with two, 6.43 with three skewed)
        if (SKEWED_HOST_RANGES) return (unsigned)std::min<size_t>(8, std::max<size_t>(3, n >> 21));
        return (unsigned)std::min<size_t>(16, std::max<size_t>(2, n >> 20));
    }

    // Window totals of a MultiExp whose scalars (and, unless `resident`, points) are in host memory: the windows of `plan`
    // over points [0, n) (registered bases: [resident_base, resident_base + n)), cut into point ranges whose copies run
    // under the pipeline of the previous range; out_totals receives plan.nwin_local totals (the ranges' totals added on the
    // host, g1JacExtended.add). `first` is leased by the caller; a second workspace is borrowed when one is free,
    // otherwise the ranges run one after the other.
    static int window_sums_from_host(Context &ctx, Workspace &first, const uint64_t *points, const ResidentBases *resident,
                                     size_t resident_base, const uint64_t *scalars, size_t n, const WindowPlan &plan,
                                     unsigned nr, Ext *out_totals) {
        const uint32_t nw = plan.nwin_local, nsets = bucket_sets(plan);
        if (nw == 0) return GMSM_OK;
        const size_t per = (n + nr - 1) / nr;
        // Range boundaries. With registered bases only the scalars cross PCIe and the device is the slower side: what the
        // call exposes of its copies is the copy of the FIRST range (nothing to compute yet), so that one is half as long
        // as the others - and so is the last one once there are many (its pipeline is the tail after the last copy).
        // Measured (profiles/r03_host_skew.log, BN254 G1 warm-bases, uniform -> skewed): 2^20 2.27 -> 2.15 ms, 2^22 6.92 -> 6.67,
        // 2^24 23.4 -> 22.5; with the bases crossing too (cold) the link is as slow as the device and uniform ranges are as
        // good as any. A forced count (GMSM_OPT_HOST_RANGES) keeps uniform ranges.
        std::vector<size_t> cut(nr + 1, 0);
        {
            const bool skew = SKEWED_HOST_RANGES && points == nullptr && nr >= 3 && options().host_ranges.load(std::memory_order_relaxed) == 0;
            std::vector<double> wgt(nr, 1.0);
            if (skew) {
                wgt[0] = 0.5;
                if (nr >= 4) wgt[nr - 1] = 0.5;
            }
            double tot = 0, run = 0;
            for (double v : wgt) tot += v;
            bool ok = true;
            for (unsigned r = 0; r < nr; ++r) {
                run += wgt[r];
                cut[r + 1] = r + 1 == nr ? n : (size_t)((double)n * run / tot);
                if (cut[r + 1] <= cut[r] || cut[r + 1] - cut[r] > max_run_points(plan)) ok = false;
            }
            if (!ok)
                for (unsigned r = 0; r <= nr; ++r) cut[r] = std::min(n, (size_t)r * per);
        }
        Workspace *w[2] = {&first, nr > 1 ? ctx.acquire(false) : nullptr};
        const unsigned nws = w[1] ? 2 : 1;
        // More than one range: every range stops after its fix-up, its bucket sums are added to the call's running buckets
        // (first.carry) on a third stream, and ONE reduction follows the last merge - a range costs its accumulation and
        // one addition per occupied bucket, not another 0.35 ms reduction chain. With one workspace the ranges and the
        // merges simply alternate on its stream.
        constexpr size_t REC = sizeof(typename OpsSerial::Mem);
        int rc = GMSM_OK;
        if (nws == 2 && (rc = first.side_stream(first.mstream))) {
            ctx.release(w[1]);
            return rc;
        }
        hipStream_t ms = nws == 2 ? first.mstream : first.stream;
        if (nr > 1 && (rc = first.carry.ensure((size_t)nsets * plan.nbuckets * REC))) {
            if (w[1]) ctx.release(w[1]);
            return rc;
        }
        for (unsigned r = 0; r < nr && rc == GMSM_OK; ++r) {
            Workspace &ws = *w[r % nws];
            const size_t lo = cut[r], len = cut[r + 1] - lo;
            const void *dp = nullptr;
            RunRequest rq;
            rq.resident_offset = resident_base + lo;
            rq.buckets_only = nr > 1;  // (one range: the whole pipeline, totals in ws.pinned)
            // hipMemcpyAsync from pageable memory returns when the caller's buffer has been consumed; the kernels
            // queued behind it do not wait for the host, so range k computes while range k+1 is being copied
            if ((rc = ws.h2d_scalars.ensure(len * SCALAR_BYTES))) break;
            if (hipMemcpyAsync(ws.h2d_scalars.ptr, (const char *)scalars + lo * SCALAR_BYTES, len * SCALAR_BYTES,
                               hipMemcpyHostToDevice, ws.stream) != hipSuccess) {
                rc = fail(GMSM_ERR_DEVICE, "hipMemcpyAsync(scalars) failed");
                break;
            }
            if (points) {
                if ((rc = ws.h2d_points.ensure(len * AFF_BYTES))) break;
                if (hipMemcpyAsync(ws.h2d_points.ptr, (const char *)points + lo * AFF_BYTES, len * AFF_BYTES,
                                   hipMemcpyHostToDevice, ws.stream) != hipSuccess) {
                    rc = fail(GMSM_ERR_DEVICE, "hipMemcpyAsync(points) failed");
                    break;
                }
                dp = ws.h2d_points.ptr;
            }
            if (nr == 1) {
                rc = enqueue_window_sums(ctx, ws, dp, ws.h2d_scalars.ptr, len, plan, ws.stream, resident, rq);
                break;
            }
            // the buckets of the range this workspace ran two ranges ago must have been merged before they are overwritten
            hipError_t he = hipSuccess;
            if (nws == 2 && r >= 2) he = hipStreamWaitEvent(ws.stream, ws.ev_merged, 0);
            if (he != hipSuccess) {
                rc = fail(GMSM_ERR_DEVICE, std::string("hipStreamWaitEvent: ") + hipGetErrorString(he));
                break;
            }
            if ((rc = enqueue_window_sums(ctx, ws, dp, ws.h2d_scalars.ptr, len, plan, ws.stream, resident, rq))) break;
            if (nws == 2) {
                he = hipEventRecord(ws.ev_buckets, ws.stream);
                if (he == hipSuccess) he = hipStreamWaitEvent(ms, ws.ev_buckets, 0);
            }
            hipLaunchKernelGGL((k_merge_buckets<OpsSerial>), dim3((plan.nbuckets + 255) / 256, nsets), dim3(256), 0, ms, first.carry.ptr,
                               (const void *)ws.buckets.ptr, (const uint32_t *)ws.starts.ptr, plan.nbuckets, r == 0 ? 1 : 0);
            if (he == hipSuccess && nws == 2) he = hipEventRecord(ws.ev_merged, ms);
            if (he == hipSuccess) he = hipGetLastError();
            if (he != hipSuccess) rc = fail(GMSM_ERR_DEVICE, std::string("multi-range merge: ") + hipGetErrorString(he));
        }
        if (rc == GMSM_OK && nr > 1) rc = enqueue_reduce(ctx, first, first.carry.ptr, plan, per, ms);
        if (rc == GMSM_OK && wait_stream(ms) != hipSuccess) rc = fail(GMSM_ERR_DEVICE, "hipStreamSynchronize failed");
        for (unsigned i = 0; i < nws; ++i) {  // nothing of this call is left running on either workspace
            (void)hipStreamSynchronize(w[i]->stream);
            if (rc == GMSM_OK && w[i]->pending_timed) StageTimer::collect(*w[i]);
            w[i]->pending_timed = false;
        }
        if (w[1]) ctx.release(w[1]);
        if (rc) return rc;
        memcpy(out_totals, first.pinned, (size_t)nw * sizeof(Ext));
        return GMSM_OK;
    }

    // Point ranges of a host-buffer call over n points: host_ranges(), more if one of them would exceed a pipeline run.
    static unsigned host_range_count(size_t n, bool with_points, const WindowPlan &plan) {
        unsigned nr = host_ranges(n, with_points);
        const size_t run = max_run_points(plan);
        if ((n + nr - 1) / nr > run) nr = (unsigned)((n + run - 1) / run);
        const size_t per = (n + nr - 1) / nr;
        return (unsigned)((n + per - 1) / per);
    }

    // MultiExp with the scalars (and, unless `resident`, the points) in host memory.
    static int multiexp_from_host(Context &ctx, Workspace &first, const uint64_t *points, const ResidentBases *resident,
                                  const uint64_t *scalars, size_t n, J *out) {
        if (small_serves(n, resident)) {  // one copy, one launch (gmsm_small.h)
            Workspace &ws = first;
            int rc;
            if ((rc = ws.h2d_scalars.ensure(n * SCALAR_BYTES))) return rc;
            HIP_TRY(hipMemcpyAsync(ws.h2d_scalars.ptr, scalars, n * SCALAR_BYTES, hipMemcpyHostToDevice, ws.stream));
            const void *dp = nullptr;
            if (points) {
                if ((rc = ws.h2d_points.ensure(n * AFF_BYTES))) return rc;
                HIP_TRY(hipMemcpyAsync(ws.h2d_points.ptr, points, n * AFF_BYTES, hipMemcpyHostToDevice, ws.stream));
                dp = ws.h2d_points.ptr;
            }
            const SmallPlan splan = small_plan(n, points ? nullptr : resident);
            if ((rc = enqueue_small(ctx, ws, dp, ws.h2d_scalars.ptr, n, splan, resident))) return rc;
            return collect_small(ws, splan, out);
        }
        const WindowPlan plan = plan_for(resident, n);  // the ranges share one bucket set and one reduction
        const unsigned c = plan.c;
        const unsigned nr = host_range_count(n, points != nullptr, plan);
        std::vector<Ext> totals(plan.nwin_total);
        int rc = window_sums_from_host(ctx, first, points, resident, 0, scalars, n, plan, nr, totals.data());
        if (rc) return rc;
        *out = fold(totals.data(), c, plan.nwin_total);
        return GMSM_OK;
    }

    // One rank's piece of a MultiExp sharded over several devices by the library itself (gmsm_multiexp_sharded and the
    // drop-in entries on a multi-GPU node; gmsm_engine.hip): host scalars [0, n) and host points or registered bases
    // [resident_base, resident_base + n), windows win_first, win_first + win_stride, ... of the c-bit decomposition;
    // out_xyzz = the nwin_local window totals. Runs on ctx's device; leases its own workspace.
    static int shard_piece(Context &ctx, const uint64_t *points, const ResidentBases *resident, size_t resident_base,
                           const uint64_t *scalars, size_t n, unsigned c, unsigned win_first, unsigned win_stride,
                           Ext *out_xyzz) {
        WindowPlan plan = make_plan(c, win_first, win_stride);
        // a point slice over bases with window tables of this width: one bucket set (the engine asks for the tables' c)
        if (resident && resident->tab_c.load() == c && win_first == 0 && plan.win_stride == 1 && options().tables.load(std::memory_order_relaxed) != 0)
            plan.shared = 1;
        if (n == 0) {
            for (uint32_t k = 0; k < plan.nwin_local; ++k) out_xyzz[k] = Ext::infinity();
            return GMSM_OK;
        }
        GMSM_LEASE_OR_FAIL(lease, ctx);
        return window_sums_from_host(ctx, *lease.w, points, resident, resident_base, scalars, n, plan,
                                     host_range_count(n, points != nullptr, plan), out_xyzz);
    }

    static int multiexp_host(const uint64_t *points, size_t n_points, const uint64_t *scalars, size_t n_scalars,
                             int nb_tasks, J *out) {
        // argument checks of (*G1Jac).MultiExp, multiexp.go:61-71
        if (n_points != n_scalars) return fail(GMSM_ERR_LEN, "len(points) != len(scalars)");
        if (nb_tasks > 1024) return fail(GMSM_ERR_CONFIG, "invalid config: config.NbTasks > 1024");
        Context *ctx;
        int rc = get_context(&ctx);
        if (rc) return rc;
        HIP_TRY(hipSetDevice(ctx->device));
        const size_t n = n_points;
        if (n == 0) {
            *out = J{F::one(), F::one(), F::zero()};
            return GMSM_OK;
        }
        GMSM_LEASE_OR_FAIL(lease, *ctx);
        return multiexp_from_host(*ctx, *lease.w, points, nullptr, scalars, n, out);
    }
};

}  // namespace gmsm

#include "gmsm_group_debug.h"
#include "gmsm_group_vtable.h"
