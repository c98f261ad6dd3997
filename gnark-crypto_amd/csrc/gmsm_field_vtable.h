// The function table of one curve's scalar field (FieldVTable, gmsm_context.h): the marshalling of the entries over Fr alone, as
// gmsm_group_vtable.h is for a group. Instantiated once per curve, in its G1 unit; VTableOf stages polynomials with it.
#pragma once
#include "gmsm_fflonk.h"    // gmsm_shplonk.h, gmsm_poly.h, gmsm_fft.h
#include "gmsm_iop_poly.h"  // gmsm_ratio.h
#include "gmsm_gkr.h"       // gmsm_iop_expr.h
#include "gmsm_fri.h"    // gmsm_mimc.h

namespace gmsm {

template <class FrP>
struct FieldVTableOf {
    // ---- KZG's evaluation and quotient (gmsm_poly.h)
    using PF = PolyField<FrP>;
    using Fr = Fp<FrP>;
    // the k polynomials on the device: host ones are staged in ws.h2d_scalars, device ones are read where they are, after
    // the work queued on the caller's stream
    static int poly_input(Workspace &ws, const uint64_t *polys, const void *d_polys, size_t total, hipStream_t caller, const Fr **out) {
        const void *in;
        int rc = stage_input(ws, ws.h2d_scalars, polys, d_polys, total * sizeof(Fr), {After::STREAM, caller}, &in);
        *out = (const Fr *)in;
        return rc;
    }
    static size_t word_slots(size_t words) { return (words * 8 + sizeof(Fr) - 1) / sizeof(Fr); }  // Fr-sized slots that hold 64-bit words
    static size_t poly_scratch(const size_t *lens, size_t k, unsigned lanes) {
        size_t s = 0;
        for (size_t i = 0; i < k; ++i) s = std::max(s, PF::scratch_elems(lens[i], lanes));
        return s;
    }
    static int poly_eval(Context &ctx, const uint64_t *polys, const void *d_polys, const size_t *lens, size_t k, const uint64_t *point,
                         hipStream_t caller, uint64_t *out_values) {
        GMSM_LEASE_OR_FAIL(lease, ctx);
        Workspace &ws = *lease.w;
        size_t total = 0;
        for (size_t i = 0; i < k; ++i) total += lens[i];
        const Fr *in;
        int rc = poly_input(ws, polys, d_polys, total, caller, &in);
        if (rc) return rc;
        const unsigned lanes = PF::lane_option();
        if ((rc = ws.poly.ensure((k + poly_scratch(lens, k, lanes)) * sizeof(Fr)))) return rc;
        Fr *vals = (Fr *)ws.poly.ptr, *scratch = vals + k;
        const FftPowers<FrP> pw = PF::powers_of(point);
        for (size_t i = 0, off = 0; i < k; off += lens[i], ++i)
            if ((rc = PF::suffix(ws.stream, pw, in + off, lens[i], nullptr, vals + i, scratch, lanes))) return rc;
        HIP_TRY(hipMemcpyAsync(out_values, vals, k * sizeof(Fr), hipMemcpyDeviceToHost, ws.stream));
        HIP_TRY(hipStreamSynchronize(ws.stream));
        return GMSM_OK;
    }
    static int poly_div(Context &ctx, const uint64_t *poly, const void *d_poly, size_t n, const uint64_t *point, hipStream_t caller,
                        uint64_t *out_h, void *d_out_h, uint64_t *out_value) {
        GMSM_LEASE_OR_FAIL(lease, ctx);
        Workspace &ws = *lease.w;
        const Fr *in;
        int rc = poly_input(ws, poly, d_poly, n, caller, &in);
        if (rc) return rc;
        if (d_out_h && poly && (rc = order_after(ws, caller))) return rc;  // the caller's stream may still use d_out_h
        const size_t hbuf = out_h ? n - 1 : 0;
        const unsigned lanes = PF::lane_option();
        if ((rc = ws.poly.ensure((1 + hbuf + PF::scratch_elems(n, lanes)) * sizeof(Fr)))) return rc;
        Fr *value = (Fr *)ws.poly.ptr, *h = out_h ? value + 1 : (Fr *)d_out_h, *scratch = value + 1 + hbuf;
        if ((rc = PF::suffix(ws.stream, PF::powers_of(point), in, n, n > 1 ? h : nullptr, value, scratch, lanes))) return rc;
        if (out_h && n > 1) HIP_TRY(hipMemcpyAsync(out_h, h, (n - 1) * sizeof(Fr), hipMemcpyDeviceToHost, ws.stream));
        if (out_value) HIP_TRY(hipMemcpyAsync(out_value, value, sizeof(Fr), hipMemcpyDeviceToHost, ws.stream));
        HIP_TRY(hipStreamSynchronize(ws.stream));
        return GMSM_OK;
    }
    // ---- the host checks of shplonk and fflonk (gmsm_fflonk.h)
    using FF = FflonkField<FrP>;
    static int open_check(const char *E, const size_t *lens, const size_t *pack_sizes, size_t k, const uint64_t *points,
                            const size_t *npoints, bool check_size, size_t registered) {
        typename FF::Plan p;
        return FF::plan(E, lens, pack_sizes, k, points, npoints, check_size, registered, &p);
    }
    // ---- fr.BatchInvert and the iop ratio polynomials (gmsm_ratio.h)
    using RF = RatioField<FrP>;
    static int fr_batch_invert(Context &ctx, const uint64_t *a, const void *d_a, size_t n, hipStream_t caller, uint64_t *out, void *d_out) {
        GMSM_LEASE_OR_FAIL(lease, ctx);
        Workspace &ws = *lease.w;
        const Fr *in;
        int rc = poly_input(ws, a, d_a, n, caller, &in);
        if (rc) return rc;
        if (d_out && a && (rc = order_after(ws, caller))) return rc;  // the caller's stream may still use d_out
        if ((rc = ws.poly.ensure((n + (out ? n : 0)) * sizeof(Fr)))) return rc;
        Fr *run = (Fr *)ws.poly.ptr, *res = out ? run + n : (Fr *)d_out;
        if ((rc = RF::invert(ws.stream, in, n, run, nullptr, res, PF::lane_option()))) return rc;
        if (out) HIP_TRY(hipMemcpyAsync(out, res, n * sizeof(Fr), hipMemcpyDeviceToHost, ws.stream));
        HIP_TRY(hipStreamSynchronize(ws.stream));
        return GMSM_OK;
    }
    // The scratch of a ratio call in ws.poly: the two factor vectors (N and D after the scan), the inversion's running
    // products, the scan's lane and tile values, then `tail` more elements for the call's small tables.
    struct RatioBuffers {
        Fr *fnum, *fden, *run, *scan, *tail;
        unsigned lanes;
    };
    static int ratio_buffers(Workspace &ws, size_t n, size_t tail, RatioBuffers *b) {
        b->lanes = PF::lane_option();
        const size_t scan = RF::scan_scratch(n, b->lanes);
        if (int rc = ws.poly.ensure((3 * n + scan + tail) * sizeof(Fr))) return rc;
        b->fnum = (Fr *)ws.poly.ptr, b->fden = b->fnum + n, b->run = b->fden + n, b->scan = b->run + n, b->tail = b->scan + scan;
        return GMSM_OK;
    }
    // The workspace's stage events are about to be recorded anew: events that an enqueue-only MultiExp left for the next call
    // to read are read now or dropped, as the MultiExp path does, so a ratio call that leaves early never hands mixed pairs on.
    static void ratio_settle_events(Workspace &ws) {
        if (!ws.uncollected) return;
        if (ws.timed && hipEventQuery(ws.events[ws.timed_level == 2 ? T_FIXUP : T_END]) == hipSuccess) StageTimer::collect(ws);
        ws.uncollected = false;
    }
    // From the factor vectors to the result: prefix products, Z = N inv0(D), the expected form, the copy-out. With profiling
    // at level 1 the call's stage times go to the slots 0 (factors), 2 (product scan), 5 (inversion and multiply) and 6 (the
    // expected form's transforms); `timer` has marked T_DECOMPOSE before the factor kernel.
    // bad != null (a permutation on the device, checked by the factor kernel): the pipeline runs on without waiting for the
    // verdict - it writes scratch only - and the one synchronise at the end brings *first_bad back with everything else; a
    // device output is written by k_ratio_publish, which writes nothing when the check failed, a host output after the verdict.
    static int ratio_finish(Workspace &ws, StageTimer &timer, FftDomain *d, const RatioBuffers &b, size_t n, int basis, int layout,
                            uint64_t *out, void *d_out, const unsigned long long *bad, unsigned long long *first_bad) {
        hipStream_t s = ws.stream;
        timer.mark(T_HIST, s), timer.mark(T_SCAN, s);
        int rc = RF::scan2(s, b.fnum, b.fden, n, b.scan, b.lanes);
        if (rc) return rc;
        timer.mark(T_SCATTER, s), timer.mark(T_ACCUMULATE, s), timer.mark(T_FIXUP, s);
        Fr *z = d_out && !bad ? (Fr *)d_out : b.fnum;
        if ((rc = RF::invert(s, b.fden, n, b.run, b.fnum, z, b.lanes))) return rc;
        timer.mark(T_REDUCE, s);
        if ((rc = RF::expected_form(s, d, z, basis, (uint32_t)layout))) return rc;
        if (bad && d_out) {
            hipLaunchKernelGGL((k_ratio_publish<FrP>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const Fr *)z, (Fr *)d_out, n, bad);
            HIP_TRY(hipGetLastError());
        }
        timer.mark(T_END, s);
        if (bad) HIP_TRY(hipMemcpyAsync(first_bad, bad, sizeof *first_bad, hipMemcpyDeviceToHost, s));
        else if (out) HIP_TRY(hipMemcpyAsync(out, z, n * sizeof(Fr), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (bad && *first_bad != ~0ull) return GMSM_OK;  // the caller refuses; nothing was written to the output
        if (bad && out) {
            HIP_TRY(hipMemcpyAsync(out, z, n * sizeof(Fr), hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
        }
        if (timer.level == 1) StageTimer::collect(ws);
        return GMSM_OK;
    }
    static int ratio_copy(Context &ctx, FftDomain *d, const uint64_t *entries, const void *d_entries, size_t m, const uint32_t *layouts,
                          const int64_t *perm, const void *d_perm, const uint64_t *beta, const uint64_t *gamma, int basis, int layout,
                          hipStream_t caller, uint64_t *out, void *d_out) {
        GMSM_LEASE_OR_FAIL(lease, ctx);
        Workspace &ws = *lease.w;
        const size_t n = (size_t)1 << d->log2n;
        const Fr *in;
        const void *pm;
        int rc = poly_input(ws, entries, d_entries, m * n, caller, &in);
        if (rc || (rc = stage_input(ws, ws.h2d_points, perm, d_perm, m * n * 8, {After::STREAM, caller}, &pm))) return rc;
        if (d_out && entries && perm && (rc = order_after(ws, caller))) return rc;  // the caller's stream may still use d_out
        const size_t lay_slots = word_slots((m + 1) / 2);
        RatioBuffers b;
        if ((rc = ratio_buffers(ws, n, m + lay_slots + 1, &b))) return rc;
        Fr *bg = b.tail;
        uint32_t *lay = (uint32_t *)(bg + m);
        unsigned long long *bad = (unsigned long long *)(bg + m + lay_slots);
        const Fr gm = fr_from_limbs<Fr>(gamma);
        std::vector<Fr> table(m);
        RF::coset_table(d, fr_from_limbs<Fr>(beta), m, table.data());
        const unsigned long long none = ~0ull;
        unsigned long long first_bad = none;
        DrainOnExit drain{ws.stream};
        HIP_TRY(hipMemcpyAsync(bg, table.data(), m * sizeof(Fr), hipMemcpyHostToDevice, ws.stream));
        HIP_TRY(hipMemcpyAsync(lay, layouts, m * sizeof(uint32_t), hipMemcpyHostToDevice, ws.stream));
        HIP_TRY(hipMemcpyAsync(bad, &none, sizeof none, hipMemcpyHostToDevice, ws.stream));
        ratio_settle_events(ws);
        StageTimer timer(ws, true);
        timer.mark(T_DECOMPOSE, ws.stream);
        hipLaunchKernelGGL((k_ratio_factors_copy<FrP>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ws.stream, in,
                           (const uint32_t *)lay, m, n, d->log2n, (const long long *)pm, (const Fr *)d->twiddles_lz.ptr, (const Fr *)bg, gm, b.fnum,
                           b.fden, bad);
        HIP_TRY(hipGetLastError());
        // a host permutation was checked before it was staged; one on the device: the factor kernel's verdict, read at the end
        if ((rc = ratio_finish(ws, timer, d, b, n, basis, layout, out, d_out, d_perm ? bad : nullptr, &first_bad))) return rc;
        if (first_bad != none) {
            long long v = 0;
            HIP_TRY(hipMemcpy(&v, (const long long *)d_perm + first_bad, sizeof v, hipMemcpyDeviceToHost));
            return fail(GMSM_ERR_ARG, ratio_perm_error((size_t)first_bad, v, m * n));
        }
        return GMSM_OK;
    }
    static int ratio_shuffled(Context &ctx, FftDomain *d, const uint64_t *num, const void *d_num, const uint64_t *den, const void *d_den,
                              size_t m, const uint32_t *num_layouts, const uint32_t *den_layouts, const uint64_t *beta, int basis, int layout,
                              hipStream_t caller, uint64_t *out, void *d_out) {
        GMSM_LEASE_OR_FAIL(lease, ctx);
        Workspace &ws = *lease.w;
        const size_t n = (size_t)1 << d->log2n;
        const Fr *pn;
        const void *pd;
        int rc = poly_input(ws, num, d_num, m * n, caller, &pn);
        if (rc || (rc = stage_input(ws, ws.h2d_points, den, d_den, m * n * sizeof(Fr), {After::STREAM, caller}, &pd))) return rc;
        if (d_out && num && den && (rc = order_after(ws, caller))) return rc;  // the caller's stream may still use d_out
        RatioBuffers b;
        if ((rc = ratio_buffers(ws, n, word_slots(m), &b))) return rc;
        uint32_t *lay = (uint32_t *)b.tail;
        const Fr bt = fr_from_limbs<Fr>(beta);
        DrainOnExit drain{ws.stream};
        HIP_TRY(hipMemcpyAsync(lay, num_layouts, m * sizeof(uint32_t), hipMemcpyHostToDevice, ws.stream));
        HIP_TRY(hipMemcpyAsync(lay + m, den_layouts, m * sizeof(uint32_t), hipMemcpyHostToDevice, ws.stream));
        ratio_settle_events(ws);
        StageTimer timer(ws, true);
        timer.mark(T_DECOMPOSE, ws.stream);
        hipLaunchKernelGGL((k_ratio_factors_shuffled<FrP>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ws.stream, pn,
                           (const Fr *)pd, (const uint32_t *)lay, m, n, d->log2n, bt, b.fnum, b.fden);
        HIP_TRY(hipGetLastError());
        return ratio_finish(ws, timer, d, b, n, basis, layout, out, d_out, nullptr, nullptr);
    }
    // ---- iop.Polynomial: basis changes, Evaluate, DivideByXMinusOne (gmsm_iop_poly.h)
    using IP = IopPolyField<FrP>;
    static int iop_to_basis(Context &ctx, FftDomain *d, uint64_t *a, void *d_a, size_t len, int basis, int layout, int to_basis,
                            hipStream_t caller, int *out_layout) {
        GMSM_LEASE_OR_FAIL(lease, ctx);
        Workspace &ws = *lease.w;
        const size_t n = (size_t)1 << d->log2n;
        Fr *v = (Fr *)d_a;
        int rc;
        DrainOnExit drain{ws.stream};
        if (a) {
            if ((rc = ws.h2d_scalars.ensure(n * sizeof(Fr)))) return rc;
            v = (Fr *)ws.h2d_scalars.ptr;
            if (len) HIP_TRY(hipMemcpyAsync(v, a, len * sizeof(Fr), hipMemcpyHostToDevice, ws.stream));
        } else if ((rc = order_after(ws, caller))) {
            return rc;
        }
        // grow (polynomial.go:351-356): the tail is zero whatever the layout, also when the basis is already the target
        if (len < n) HIP_TRY(hipMemsetAsync(v + len, 0, (n - len) * sizeof(Fr), ws.stream));
        {
            std::lock_guard<std::mutex> lk(d->mu);
            rc = IP::to_basis(ws.stream, d, v, basis, layout, to_basis, out_layout);
        }
        if (rc) return rc;
        if (a) HIP_TRY(hipMemcpyAsync(a, v, n * sizeof(Fr), hipMemcpyDeviceToHost, ws.stream));
        HIP_TRY(hipStreamSynchronize(ws.stream));
        return GMSM_OK;
    }
    static int iop_evaluate(Context &ctx, const uint64_t *polys, const void *d_polys, size_t k, size_t len, size_t size, int basis,
                            const uint32_t *layouts, unsigned shift, const uint64_t *coset, const uint64_t *x, hipStream_t caller,
                            uint64_t *out_values) {
        const Fr xx = IP::effective_point(x, basis, coset, shift, size);
        GMSM_LEASE_OR_FAIL(lease, ctx);
        Workspace &ws = *lease.w;
        const Fr *in;
        int rc = poly_input(ws, polys, d_polys, k * len, caller, &in);
        if (rc) return rc;
        const unsigned lanes = PF::lane_option();
        DrainOnExit drain{ws.stream};
        Fr *vals;
        if (basis == IOP_CANONICAL) {
            if ((rc = ws.poly.ensure((k + PF::scratch_elems(len, lanes)) * sizeof(Fr)))) return rc;
            vals = (Fr *)ws.poly.ptr;
            const FftPowers<FrP> pw = FftField<FrP>::powers_of(xx);
            for (size_t j = 0; j < k; ++j)
                if ((rc = IP::eval_canonical(ws.stream, pw, in + j * len, len, layouts[j] == IOP_BIT_REVERSE, vals + j, vals + k, lanes))) return rc;
        } else {
            unsigned log2len = 0;
            while (((size_t)1 << log2len) < len) ++log2len;
            const size_t part = IP::bary_scratch(k, len, lanes);
            if ((rc = ws.poly.ensure((k + part + word_slots((k + 1) / 2)) * sizeof(Fr)))) return rc;
            vals = (Fr *)ws.poly.ptr;
            uint32_t *lay = (uint32_t *)(vals + k + part);
            HIP_TRY(hipMemcpyAsync(lay, layouts, k * sizeof(uint32_t), hipMemcpyHostToDevice, ws.stream));
            if ((rc = IP::barycentric(ws.stream, in, (const uint32_t *)lay, k, len, log2len, xx, vals + k, vals, lanes))) return rc;
        }
        HIP_TRY(hipMemcpyAsync(out_values, vals, k * sizeof(Fr), hipMemcpyDeviceToHost, ws.stream));
        HIP_TRY(hipStreamSynchronize(ws.stream));
        return GMSM_OK;
    }
    static int iop_quotient(Context &ctx, FftDomain *small, FftDomain *big, const uint64_t *a, const void *d_a, int layout, size_t shift,
                            hipStream_t caller, uint64_t *out, void *d_out) {
        GMSM_LEASE_OR_FAIL(lease, ctx);
        Workspace &ws = *lease.w;
        const size_t N = (size_t)1 << big->log2n, rho = N >> small->log2n;
        const Fr *in;
        int rc = poly_input(ws, a, d_a, N, caller, &in);
        if (rc) return rc;
        if (d_out && a && (rc = order_after(ws, caller))) return rc;  // the caller's stream may still use d_out
        if ((rc = ws.poly.ensure((rho + (out ? N : 0)) * sizeof(Fr)))) return rc;
        Fr *run = (Fr *)ws.poly.ptr, *res = out ? run + rho : (Fr *)d_out;
        DrainOnExit drain{ws.stream};
        {
            std::lock_guard<std::mutex> lk(big->mu);
            rc = IP::quotient(ws.stream, big, small->log2n, in, layout == (int)IOP_BIT_REVERSE, shift * rho, run, res, PF::lane_option());
        }
        if (rc) return rc;
        if (out) HIP_TRY(hipMemcpyAsync(out, res, N * sizeof(Fr), hipMemcpyDeviceToHost, ws.stream));
        HIP_TRY(hipStreamSynchronize(ws.stream));
        return GMSM_OK;
    }
    // ---- iop.Evaluate of a straight-line program (gmsm_iop_expr.h). ws.poly holds the result of a host-output call, then the
    // call's small tables in one piece: the constants, the input descriptors, the program.
    using IE = IopExprField<FrP>;
    static int iop_expr(Context &ctx, FftDomain *d, const uint32_t *prog, size_t prog_len, unsigned nregs, const uint64_t *consts, size_t n_consts,
                        const uint64_t *const *polys, const void *const *d_polys, size_t m, size_t len, const size_t *offsets,
                        const uint32_t *layouts, int out_layout, hipStream_t caller, uint64_t *out, void *d_out) {
        GMSM_LEASE_OR_FAIL(lease, ctx);
        Workspace &ws = *lease.w;
        int rc;
        if ((d_polys || d_out) && (rc = order_after(ws, caller))) return rc;  // inputs produced there; it may still use d_out
        const size_t desc_at = n_consts * sizeof(Fr), prog_at = desc_at + m * sizeof(ExprInput), tab_bytes = prog_at + prog_len * sizeof(uint32_t);
        const size_t res_bytes = out ? len * sizeof(Fr) : 0;
        if ((rc = ws.poly.ensure(res_bytes + tab_bytes))) return rc;
        if (polys && (rc = ws.h2d_scalars.ensure(m * len * sizeof(Fr)))) return rc;
        unsigned char *dtab = (unsigned char *)ws.poly.ptr + res_bytes;
        Fr *res = out ? (Fr *)ws.poly.ptr : (Fr *)d_out;
        std::vector<unsigned char> tab(tab_bytes);
        if (n_consts) memcpy(tab.data(), consts, n_consts * sizeof(Fr));
        for (size_t j = 0; j < m; ++j) {
            ExprInput in;
            in.ptr = polys ? (const void *)((const Fr *)ws.h2d_scalars.ptr + j * len) : d_polys[j];
            in.offset = offsets[j], in.rev = layouts[j] == IOP_BIT_REVERSE ? 1u : 0u, in.pad = 0;
            memcpy(tab.data() + desc_at + j * sizeof(ExprInput), &in, sizeof in);
        }
        memcpy(tab.data() + prog_at, prog, prog_len * sizeof(uint32_t));
        DrainOnExit drain{ws.stream};
        if (polys)
            for (size_t j = 0; j < m; ++j)
                HIP_TRY(hipMemcpyAsync((Fr *)ws.h2d_scalars.ptr + j * len, polys[j], len * sizeof(Fr), hipMemcpyHostToDevice, ws.stream));
        HIP_TRY(hipMemcpyAsync(dtab, tab.data(), tab_bytes, hipMemcpyHostToDevice, ws.stream));
        ratio_settle_events(ws);
        StageTimer timer(ws, true);
        timer.mark(T_DECOMPOSE, ws.stream);
        const Fr *tw = d && len > 1 ? (const Fr *)d->twiddles_lz.ptr : nullptr;  // built with the domain, read-only since
        if ((rc = IE::run(ws.stream, (const uint32_t *)(dtab + prog_at), prog_len, nregs, (const Fr *)dtab, (const ExprInput *)(dtab + desc_at), tw, len,
                          out_layout == (int)IOP_BIT_REVERSE, res)))
            return rc;
        for (int ev = T_HIST; ev <= T_END; ++ev) timer.mark(ev, ws.stream);  // the kernel's time goes to slot 0, nothing to the others
        if (out) HIP_TRY(hipMemcpyAsync(out, res, len * sizeof(Fr), hipMemcpyDeviceToHost, ws.stream));
        HIP_TRY(hipStreamSynchronize(ws.stream));
        if (timer.level == 1) StageTimer::collect(ws);
        return GMSM_OK;
    }
    // ---- fr/polynomial.MultiLin and one GKR sumcheck claim (gmsm_gkr.h)
    using GK = GkrField<FrP>;
    static constexpr auto multilin_fold = &GK::multilin_fold;
    static constexpr auto multilin_evaluate = &GK::multilin_evaluate;
    static constexpr auto multilin_eq = &GK::multilin_eq;
    static constexpr auto gkr_new = &GK::gkr_new;
    static constexpr auto gkr_next = &GK::gkr_next;
    static constexpr auto gkr_final = &GK::gkr_final;
    // ---- fr/mimc and the Merkle tree over it (gmsm_mimc.h)
    using MF = MimcField<FrP>;
    static constexpr auto mimc_constants = &MF::constants;
    static constexpr auto mimc_hash = &MF::hash;
    static constexpr auto mimc_sum_batch = &MF::sum_batch;
    static constexpr auto merkle_new = &MF::merkle_new;
    static constexpr auto merkle_prove = &MF::merkle_prove;
    // ---- fr/fri's prover over both (gmsm_fri.h)
    using FR = FriField<FrP>;
    static constexpr auto fri_commit = &FR::commit;
    static constexpr auto fri_fold = &FR::fold;
    static constexpr auto fri_layer = &FR::layer;
    static constexpr auto fri_query = &FR::query;
    static const FieldVTable *get() {
        static const FieldVTable vt = [] {  // filled by name, in the order of the struct's members, as VTableOf::get() is
            FieldVTable v{};
            v.scalar_bytes = sizeof(Fr), v.fr_bits = FrP::BITS, v.fr_max_order = (unsigned)FrP::MAX_ORDER;
            // fr/fft and the divisor search need no marshalling: the typed entry points have the table's signatures
            v.fft_domain_new = &FftField<FrP>::domain_new, v.fft_run = &FftField<FrP>::run, v.fft_bit_reverse = &FftField<FrP>::bit_reverse;
            v.fflonk_next_divisor = &FF::next_divisor;
#define GMSM_VT(f) v.f = f
            GMSM_VT(poly_eval), GMSM_VT(poly_div), GMSM_VT(open_check), GMSM_VT(fr_batch_invert), GMSM_VT(ratio_copy), GMSM_VT(ratio_shuffled);
            GMSM_VT(iop_to_basis), GMSM_VT(iop_evaluate), GMSM_VT(iop_quotient), GMSM_VT(iop_expr);
            GMSM_VT(multilin_fold), GMSM_VT(multilin_evaluate), GMSM_VT(multilin_eq), GMSM_VT(gkr_new), GMSM_VT(gkr_next), GMSM_VT(gkr_final);
            v.mimc_rounds = FrP::MIMC_ROUNDS;
            GMSM_VT(mimc_constants), GMSM_VT(mimc_hash), GMSM_VT(mimc_sum_batch), GMSM_VT(merkle_new), GMSM_VT(merkle_prove);
            GMSM_VT(fri_commit), GMSM_VT(fri_fold), GMSM_VT(fri_layer), GMSM_VT(fri_query);
#undef GMSM_VT
            return v;
        }();
        return &vt;
    }
};

}  // namespace gmsm
