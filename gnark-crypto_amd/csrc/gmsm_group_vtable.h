// The function table of one (curve, group): what the C ABI (gmsm_engine.hip) dispatches through - argument marshalling
// between the ABI's uint64_t limbs / void pointers and the typed entry points of struct Group. Included by gmsm_group.h.
#pragma once
#include "gmsm_group.h"
#include "gmsm_group_debug.h"

namespace gmsm {

// ------------------------------------------------------------------ function table

template <class G, bool IS_G1>
struct VTableOf {
    static int multiexp_host(const uint64_t *points, size_t n_points, const uint64_t *scalars, size_t n_scalars,
                             int nb_tasks, uint64_t *out_jac) {
        typename G::J j;
        int rc = G::multiexp_host(points, n_points, scalars, n_scalars, nb_tasks, &j);
        if (rc) return rc;
        memcpy(out_jac, &j, sizeof j);
        return GMSM_OK;
    }
    static int multiexp_device(Context &ctx, const void *d_points, const void *d_scalars, size_t n, hipStream_t stream,
                               uint64_t *out_jac, const ResidentBases *resident) {
        typename G::J j;
        if (n == 0) j = typename G::J{G::F::one(), G::F::one(), G::F::zero()};
        else {
            GMSM_LEASE_OR_FAIL(lease, ctx);
            int rc = G::multiexp_device(ctx, *lease.w, d_points, d_scalars, n, stream, &j, resident);
            if (rc) return rc;
        }
        memcpy(out_jac, &j, sizeof j);
        return GMSM_OK;
    }
    static int multiexp_bases_host(Context &ctx, const uint64_t *scalars, size_t n, uint64_t *out_jac,
                                   const ResidentBases *resident) {
        GMSM_LEASE_OR_FAIL(lease, ctx);
        typename G::J j;
        int rc = G::multiexp_from_host(ctx, *lease.w, nullptr, resident, scalars, n, &j);
        if (rc) return rc;
        memcpy(out_jac, &j, sizeof j);
        return GMSM_OK;
    }
    static int shard_piece(Context &ctx, const uint64_t *points, const ResidentBases *resident, size_t resident_base,
                           const uint64_t *scalars, size_t n, unsigned c, unsigned win_first, unsigned win_stride,
                           uint64_t *out_xyzz) {
        return G::shard_piece(ctx, points, resident, resident_base, scalars, n, c, win_first, win_stride,
                              reinterpret_cast<typename G::Ext *>(out_xyzz));
    }
    static unsigned host_piece_ranges(size_t n, bool with_points) { return G::host_range_count(n, with_points, G::plan_for(nullptr, n)); }
    static int precompute_tables(Context &ctx, Workspace &ws, ResidentBases *rb, unsigned c) {
        return G::precompute_tables(ctx, ws, rb, c);
    }
    static bool tables_serve(size_t n_registered, size_t n_call) { return G::tables_serve(n_registered, n_call); }
    static int window_sums(Context &ctx, const void *d_points, const void *d_scalars, size_t n, unsigned c,
                           unsigned win_first, unsigned win_stride, hipStream_t stream, uint64_t *out_xyzz,
                           const ResidentBases *resident) {
        WindowPlan plan = G::make_plan(c, win_first, win_stride);
        GMSM_LEASE_OR_FAIL(lease, ctx);
        return G::window_sums(ctx, *lease.w, d_points, d_scalars, n, plan, stream,
                              reinterpret_cast<typename G::Ext *>(out_xyzz), resident);
    }
    static int register_bases(Context &ctx, const void *d_points, size_t n, hipStream_t stream, ResidentBases *out) {
        return G::register_bases(ctx, d_points, n, stream, out);
    }
    static int window_sums_enqueue(Context &ctx, const void *d_points, const void *d_scalars, size_t n, unsigned c,
                                   unsigned win_first, unsigned win_stride, hipStream_t stream, void *d_out_xyzz,
                                   const std::shared_ptr<ResidentBases> &resident) {
        WindowPlan plan = G::make_plan(c, win_first, win_stride);
        // leased for the duration of this call only: the work it leaves in flight is protected by stream order
        // (Workspace::last_use, honoured by whoever leases the workspace next), not by the lease
        GMSM_LEASE_OR_FAIL(lease, ctx);
        Workspace *ws = lease.w;
        RunRequest rq;
        rq.d_out = d_out_xyzz;
        int rc = G::enqueue_window_sums(ctx, *ws, d_points, d_scalars, n, plan, stream, resident.get(), rq);
        ws->bases_ref = resident;             // alive until the next call on this workspace replaces it
        ws->uncollected = ws->pending_timed;  // nobody waits for this call: its stage events are read by the next one
        ws->pending_timed = false;
        return rc;
    }
    static void fold_sets(const uint64_t *xyzz_sets, unsigned nsets, unsigned c, uint64_t *out_jac) {
        typename G::J j = G::fold_sets(reinterpret_cast<const typename G::Ext *>(xyzz_sets), nsets, c);
        memcpy(out_jac, &j, sizeof j);
    }
    static void fold_powers(const uint64_t *coeff, size_t n, uint64_t *out_scalars) { G::fold_powers(coeff, n, out_scalars); }
    // host or device scalars / results; exactly one of each pair is given
    static int batch_scalar_mul(Context &ctx, const uint64_t *base, const uint64_t *scalars, const void *d_scalars, size_t n,
                                hipStream_t caller_stream, uint64_t *out, void *d_out) {
        GMSM_LEASE_OR_FAIL(lease, ctx);
        Workspace &ws = *lease.w;
        int rc = order_after(ws, caller_stream);
        if (rc) return rc;
        const void *dsc;  // (the caller's stream has been ordered above, whichever side the scalars are on)
        if ((rc = stage_input(ws, ws.h2d_scalars, scalars, d_scalars, n * G::SCALAR_BYTES, {After::NOTHING}, &dsc))) return rc;
        void *dres = d_out;
        if (out && n) {
            if ((rc = ws.parted.ensure(n * G::AFF_BYTES))) return rc;
            dres = ws.parted.ptr;
        }
        if ((rc = G::batch_scalar_mul(ctx, ws, base, dsc, n, dres))) return rc;
        if (out && n) HIP_TRY(hipMemcpyAsync(out, dres, n * G::AFF_BYTES, hipMemcpyDeviceToHost, ws.stream));
        HIP_TRY(hipStreamSynchronize(ws.stream));
        return GMSM_OK;
    }
    static int batch_jac_to_affine(Context &ctx, const uint64_t *jac, size_t n, uint64_t *out) {
        if (n == 0) return GMSM_OK;
        GMSM_LEASE_OR_FAIL(lease, ctx);
        Workspace &ws = *lease.w;
        int rc;
        if ((rc = ws.h2d_points.ensure(n * sizeof(typename G::J)))) return rc;
        if ((rc = ws.parted.ensure(n * G::AFF_BYTES))) return rc;
        HIP_TRY(hipMemcpyAsync(ws.h2d_points.ptr, jac, n * sizeof(typename G::J), hipMemcpyHostToDevice, ws.stream));
        if ((rc = G::batch_jac_to_affine(ws, ws.h2d_points.ptr, n, ws.parted.ptr))) return rc;
        HIP_TRY(hipMemcpyAsync(out, ws.parted.ptr, n * G::AFF_BYTES, hipMemcpyDeviceToHost, ws.stream));
        HIP_TRY(hipStreamSynchronize(ws.stream));
        return GMSM_OK;
    }
    static int submit(Context &ctx, Workspace &ws, const void *d_scalars, size_t n, const ResidentBases *resident) {
        return G::multiexp_submit(ctx, ws, d_scalars, n, resident);
    }
    static int decode_raw(Workspace &ws, const void *d_raw, size_t n, int level, void *d_out, long long *bad_index,
                          uint32_t *status) {
        return G::decode_raw(ws, d_raw, n, level, d_out, bad_index, status);
    }
    static int decode_compressed(Workspace &ws, const void *d_comp, size_t n, int level, void *d_out, long long *bad_index,
                                 uint32_t *status) {
        return G::decode_compressed(ws, d_comp, n, level, d_out, bad_index, status);
    }
    static int encode_compressed(Workspace &ws, const void *d_points, size_t n, void *d_comp) {
        return G::encode_compressed(ws, d_points, n, d_comp);
    }
    static int fft_domain_new(Context &ctx, hipStream_t stream, unsigned log2n, FftDomain *out) {
        return FftField<typename G::FrP>::domain_new(ctx, stream, log2n, out);
    }
    static int fft_run(hipStream_t stream, FftDomain *d, void *d_a, bool inverse, bool dif, bool coset) {
        return FftField<typename G::FrP>::run(stream, d, d_a, inverse, dif, coset);
    }
    static int fft_bit_reverse(hipStream_t stream, void *d_a, size_t n) {
        return FftField<typename G::FrP>::bit_reverse(stream, d_a, n);
    }
    static int validate_points(Workspace &ws, const void *d_points, size_t n, int level, long long *bad_index,
                               uint32_t *status) {
        return G::validate_points(ws, d_points, n, level, bad_index, status);
    }
    static int collect(Workspace &ws, uint64_t *out_jac) {
        typename G::J j;
        int rc = G::multiexp_collect(ws, &j);
        if (rc) return rc;
        memcpy(out_jac, &j, sizeof j);
        return GMSM_OK;
    }
    static void fold(const uint64_t *xyzz_windows, unsigned c, uint64_t *out_jac) {
        typename G::J j = G::fold(reinterpret_cast<const typename G::Ext *>(xyzz_windows), c);
        memcpy(out_jac, &j, sizeof j);
    }
    static void jac_to_affine(const uint64_t *jac, uint64_t *out_affine) {
        typename G::J j;
        memcpy(&j, jac, sizeof j);
        typename G::Aff a = affine_from_jac(j);
        memcpy(out_affine, &a, sizeof a);
    }
    static int debug_decompose(const uint64_t *scalars, size_t n, unsigned c, uint32_t *out_digits) {
        return debug_decompose_impl<G>(scalars, n, c, out_digits);
    }
    static int debug_glv_split(const uint64_t *scalars, size_t n, uint32_t *out) { return debug_glv_split_impl<G>(scalars, n, out); }
    // what a MultiExp over n bases taken anew runs as (gmsm_default_plan)
    static void plan_info(size_t n, unsigned *c, unsigned *nwin, unsigned *entries_per_point, unsigned *fused) {
        if (G::small_serves(n, nullptr)) {
            const typename G::SmallPlan sp = G::small_plan(n, nullptr);
            *c = sp.plan.c, *nwin = sp.plan.nwin_total, *entries_per_point = sp.glv ? 2u : 1u, *fused = 1u;
            return;
        }
        const WindowPlan p = G::plan_for(nullptr, n);
        *c = p.c, *nwin = p.nwin_total, *entries_per_point = p.glv ? 2u : 1u, *fused = 0u;
    }
    static void reduce_shape(const Context &ctx, uint32_t nw, uint32_t nbuckets, uint32_t out[6]) { G::reduce_shape(ctx.num_cus, nw, nbuckets, out); }
    // gmsm_debug_run_layout: Pipeline::plan_run, no device; flags = resident | d_out << 1 | buckets_only << 2 | tail_mode << 3
    static int run_layout(int num_cus, size_t n, unsigned c, unsigned win_first, unsigned win_stride, bool glv, bool shared,
                          unsigned flags, uint64_t *out) {
        if (glv && !G::glv_width_built(c)) return fail(GMSM_ERR_ARG, "gmsm_debug_run_layout: no GLV decomposition of this width");
        WindowPlan plan = glv ? G::make_plan_glv(c, win_first, win_stride) : G::make_plan(c, win_first, win_stride);
        plan.shared = shared ? 1 : 0;
        RunRequest rq;
        rq.d_out = (flags & 2u) ? out : nullptr;  // (only its presence shapes the layout)
        rq.buckets_only = (flags & 4u) != 0;
        rq.tail_mode = (int)((flags >> 3) & 3u);
        if (plan.nwin_local == 0) return fail(GMSM_ERR_ARG, "gmsm_debug_run_layout: no window in this piece");
        const typename G::RunLayout layout = G::plan_run(num_cus, plan, n, (flags & 1u) != 0, rq);
        if (layout.error) return fail(GMSM_ERR_ARG, layout.error);
        G::flatten(num_cus, layout, out);
        return GMSM_OK;
    }
    static void fold_planes(const uint64_t *planes, unsigned c, unsigned nwin, unsigned log2L, unsigned nhigh, uint64_t *out_jac) {
        typename G::J j = G::fold_planes(reinterpret_cast<const typename G::Ext *>(planes), c, nwin, log2L, nhigh);
        memcpy(out_jac, &j, sizeof j);
    }
    static int debug_field_op(int field, int op, const uint64_t *a, const uint64_t *b, size_t count, uint64_t *out) {
        using BaseP = typename G::F::Params;
        if (field == 0) {
            if (op == 6) return debug_from_mont<BaseP>(a, count, out);
            return debug_field<Fp<BaseP>>(op, a, b, count, out);
        } else if (field == 1) {
            if (op == 6) return debug_from_mont<typename G::FrP>(a, count, out);
            return debug_field<Fp<typename G::FrP>>(op, a, b, count, out);
        }
        if (op == 6) return fail(GMSM_ERR_ARG, "from_mont is defined on prime fields only");
        if (field == 3) {  // coordinate field through the lazy-limb code
            using U = typename G::U;
            using S = typename LzTraits<U>::Sat;
            return run_elementwise<S>(count * sizeof(S), a, b ? count * sizeof(S) : 0, b, count * sizeof(S), out,
                                      [&](void *da, void *db, void *dout, hipStream_t s) {
                                          hipLaunchKernelGGL((k_lazy_field_op<U>), dim3((unsigned)((count + 63) / 64)), dim3(64),
                                                             0, s, op, (const S *)da, (const S *)db, count, (S *)dout);
                                      });
        }
        return debug_field<typename G::F>(op, a, b, count, out);
    }
    static int debug_group_op(int op, const uint64_t *acc, const uint64_t *other, size_t count, uint64_t *out) {
        if (op >= 4) {  // 4..7 = ops 0..3 through the lazy-limb group law
            using U = typename G::U;
            using F = typename G::F;
            const int lop = op - 4;
            const size_t ob = (lop == 0 || lop == 1) ? sizeof(Affine<F>) : sizeof(XYZZ<F>);
            return run_elementwise<F>(count * sizeof(XYZZ<F>), acc, other ? count * ob : 0, other, count * sizeof(XYZZ<F>), out,
                                      [&](void *da, void *db, void *dout, hipStream_t s) {
                                          hipLaunchKernelGGL((k_lazy_group_op<U>), dim3((unsigned)((count + 63) / 64)), dim3(64),
                                                             0, s, lop, (const XYZZ<F> *)da, (const void *)db, count,
                                                             (XYZZ<F> *)dout);
                                      });
        }
        return debug_group<G>(op, acc, other, count, out);
    }
    static void generate_points(const uint64_t *base, const uint64_t *k0, const uint64_t *k1, int klimbs, size_t n,
                                int nthreads, uint64_t *out) {
        G::generate_points(base, k0, k1, klimbs, n, nthreads, out);
    }
    // ---- KZG opening (gmsm_poly.h)
    using PF = PolyField<typename G::FrP>;
    using Fr = Fp<typename G::FrP>;
    static_assert(sizeof(Fr) == G::SCALAR_BYTES, "fr.Element layout");
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
        const FftPowers<typename G::FrP> pw = PF::powers_of(point);
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
    static int kzg_open(Context &ctx, const uint64_t *polys, const void *d_polys, const size_t *lens, size_t k, const uint64_t *point,
                        const uint64_t *gamma, hipStream_t caller, uint64_t *out_claimed, uint64_t *out_jac, const ResidentBases *resident) {
        GMSM_LEASE_OR_FAIL(lease, ctx);
        Workspace &ws = *lease.w;
        size_t total = 0, maxlen = 0;
        for (size_t i = 0; i < k; ++i) total += lens[i], maxlen = std::max(maxlen, lens[i]);
        const Fr *in;
        int rc = poly_input(ws, polys, d_polys, total, caller, &in);
        if (rc) return rc;
        const bool folds = k > 1;
        const size_t ol_elems = folds ? word_slots(2 * k) : 0;
        const unsigned lanes = PF::lane_option();
        const size_t elems = 1 + (maxlen - 1) + (folds ? maxlen : 0) + ol_elems + PF::scratch_elems(maxlen, lanes);
        if ((rc = ws.poly.ensure(elems * sizeof(Fr)))) return rc;
        Fr *value = (Fr *)ws.poly.ptr, *h = value + 1, *folded = h + (maxlen - 1);
        uint64_t *off_len = (uint64_t *)(folded + (folds ? maxlen : 0));
        Fr *scratch = folded + (folds ? maxlen : 0) + ol_elems;
        const Fr *v = in;
        if (folds) {
            if ((rc = PF::fold(ws.stream, in, lens, k, maxlen, gamma, off_len, folded))) return rc;
            v = folded;
        }
        if ((rc = PF::suffix(ws.stream, PF::powers_of(point), v, maxlen, h, value, scratch, lanes))) return rc;
        if (out_claimed) HIP_TRY(hipMemcpyAsync(out_claimed, value, sizeof(Fr), hipMemcpyDeviceToHost, ws.stream));
        // the quotient is committed where it is: the resident MultiExp over the first maxlen - 1 bases
        typename G::J j;
        if ((rc = G::multiexp_device(ctx, ws, nullptr, h, maxlen - 1, ws.stream, &j, resident))) return rc;
        HIP_TRY(hipStreamSynchronize(ws.stream));
        memcpy(out_jac, &j, sizeof j);
        return GMSM_OK;
    }
    // ---- shplonk.BatchOpen, and fflonk Fold, FoldAndCommit, BatchOpen (gmsm_fflonk.h, gmsm_shplonk.h)
    using SF = ShplonkField<typename G::FrP>;
    static typename G::J commit_or_infinity(Context &ctx, Workspace &ws, const Fr *scalars, size_t n, const ResidentBases *resident, int *rc) {
        typename G::J j{G::F::one(), G::F::one(), G::F::zero()};  // Commit of the zero polynomial
        *rc = n ? G::multiexp_device(ctx, ws, nullptr, scalars, n, ws.stream, &j, resident) : GMSM_OK;
        return j;
    }
    using FF = FflonkField<typename G::FrP>;
    static bool fflonk_next_divisor(size_t n, size_t *t) { return FF::next_divisor(n, t); }
    static int open_check(const char *E, const size_t *lens, const size_t *pack_sizes, size_t k, const uint64_t *points,
                            const size_t *npoints, bool check_size, size_t registered) {
        typename FF::Plan p;
        return FF::plan(E, lens, pack_sizes, k, points, npoints, check_size, registered, &p);
    }
    static int fflonk_fold(Context &ctx, const uint64_t *polys, const void *d_polys, const size_t *lens, size_t npolys, hipStream_t caller,
                           uint64_t *out, void *d_out, const ResidentBases *resident, uint64_t *out_jac) {
        typename FF::Plan p;
        int rc = FF::plan("gmsm_fflonk_fold", lens, &npolys, 1, nullptr, nullptr, false, 0, &p);
        if (rc) return rc;
        GMSM_LEASE_OR_FAIL(lease, ctx);
        Workspace &ws = *lease.w;
        const Fr *in;
        if ((rc = poly_input(ws, polys, d_polys, p.total, caller, &in))) return rc;
        if (d_out && polys && (rc = order_after(ws, caller))) return rc;  // the caller's stream may still use d_out
        const size_t head = word_slots(p.table_words()), fbuf = d_out ? 0 : p.maxfold;
        if ((rc = ws.poly.ensure((head + fbuf) * sizeof(Fr)))) return rc;
        std::vector<uint64_t> tbl(p.table_words());
        FF::tables(p, lens, tbl.data());
        Fr *folded = d_out ? (Fr *)d_out : (Fr *)ws.poly.ptr + head;
        HIP_TRY(hipMemcpyAsync(ws.poly.ptr, tbl.data(), tbl.size() * 8, hipMemcpyHostToDevice, ws.stream));
        if ((rc = FF::fold(ws.stream, in, (const uint64_t *)ws.poly.ptr, npolys, p.t[0], p.maxfold, folded))) return rc;
        if (out) HIP_TRY(hipMemcpyAsync(out, folded, p.maxfold * sizeof(Fr), hipMemcpyDeviceToHost, ws.stream));
        typename G::J j{G::F::one(), G::F::one(), G::F::zero()};
        // the folded polynomial is committed where it is: the resident MultiExp over the folded length
        if (resident && (rc = G::multiexp_device(ctx, ws, nullptr, folded, p.maxfold, ws.stream, &j, resident))) return rc;
        HIP_TRY(hipStreamSynchronize(ws.stream));  // `tbl` is pageable host memory: alive until here
        if (out_jac) memcpy(out_jac, &j, sizeof j);
        return GMSM_OK;
    }
    // The two halves of an opening. pack_sizes == null: shplonk's singleton form (out_folded_claimed is not written). The
    // engine's check has run the same plan, so it refuses nothing here and the entry's name is not needed for a text.
    static int open_w(Context &ctx, const uint64_t *polys, const void *d_polys, const size_t *lens, const size_t *pack_sizes, size_t k,
                      const uint64_t *points, const size_t *npoints, const uint64_t *gamma, hipStream_t caller, uint64_t *out_claimed,
                      uint64_t *out_folded_claimed, uint64_t *out_w, void *d_out_w, uint64_t *out_jac, const ResidentBases *resident) {
        typename FF::Plan p;
        int rc = FF::plan("open_w", lens, pack_sizes, k, points, npoints, true, resident->n, &p);
        if (rc) return rc;
        GMSM_LEASE_OR_FAIL(lease, ctx);
        Workspace &ws = *lease.w;
        const Fr *in;
        if ((rc = poly_input(ws, polys, d_polys, p.total, caller, &in))) return rc;
        if (d_out_w && polys && (rc = order_after(ws, caller))) return rc;  // the caller's stream may still use d_out_w
        const size_t wbuf = out_w ? p.maxfold : 0, ping = p.maxmember - 1;
        const unsigned lanes = PF::lane_option();
        const size_t scratch_elems = SF::chain_scratch(lens, p.member_points.data(), p.npolys, lanes);
        if ((rc = ws.poly.ensure((p.nrem + wbuf + 2 * ping + scratch_elems) * sizeof(Fr)))) return rc;
        Fr *rem = (Fr *)ws.poly.ptr, *w = out_w ? rem + p.nrem : (Fr *)d_out_w, *a = rem + p.nrem + wbuf, *b = a + ping, *scratch = b + ping;
        Fr g;
        memcpy(&g, gamma, sizeof g);
        if ((rc = FF::chains(ws.stream, p, in, lens, g, rem, w, a, b, scratch, lanes))) return rc;
        std::vector<Fr> d(p.nrem);
        HIP_TRY(hipMemcpyAsync(d.data(), rem, p.nrem * sizeof(Fr), hipMemcpyDeviceToHost, ws.stream));
        if (out_w) HIP_TRY(hipMemcpyAsync(out_w, w, p.maxfold * sizeof(Fr), hipMemcpyDeviceToHost, ws.stream));
        // w is committed where it is: the resident MultiExp over its true length
        const typename G::J j = commit_or_infinity(ctx, ws, w, p.wlen, resident, &rc);
        if (rc) return rc;
        HIP_TRY(hipStreamSynchronize(ws.stream));
        FF::claimed_values(p, d.data(), (Fr *)out_claimed, (Fr *)out_folded_claimed);
        memcpy(out_jac, &j, sizeof j);
        return GMSM_OK;
    }
    static int open_wprime(Context &ctx, const uint64_t *polys, const void *d_polys, const size_t *lens, const size_t *pack_sizes, size_t k,
                           const uint64_t *points, const size_t *npoints, const uint64_t *folded_claimed, const uint64_t *gamma,
                           const uint64_t *w, const void *d_w, const uint64_t *z, hipStream_t caller, uint64_t *out_jac,
                           const ResidentBases *resident) {
        typename FF::Plan p;
        int rc = FF::plan("open_wprime", lens, pack_sizes, k, points, npoints, true, resident->n, &p);
        if (rc) return rc;
        GMSM_LEASE_OR_FAIL(lease, ctx);
        Workspace &ws = *lease.w;
        const Fr *in;
        if ((rc = poly_input(ws, polys, d_polys, p.total, caller, &in))) return rc;
        if (d_w && polys && (rc = order_after(ws, caller))) return rc;  // d_w is the caller's stream's
        // host part: shplonk's c_i, Z_T(z), sum_i c_i r_i(z) over the extended sets and the inner claimed values (singleton
        // form: the sets and the claimed values as given), then the index tables, in one staging vector of Fr-sized slots
        const size_t head = k + 2 + word_slots(p.table_words());
        std::vector<Fr> stage(head);
        Fr g, zz;
        memcpy(&g, gamma, sizeof g);
        memcpy(&zz, z, sizeof zz);
        SF::combine_coefficients(p.ext.data(), p.ext_npoints.data(), k, (const Fr *)folded_claimed, g, zz, stage.data());
        FF::tables(p, lens, (uint64_t *)(stage.data() + k + 2));
        const size_t n = p.maxfold, wbuf = w ? n : 0;
        const unsigned lanes = PF::lane_option();
        if ((rc = ws.poly.ensure((head + wbuf + n + (n - 1) + PF::scratch_elems(n, lanes)) * sizeof(Fr)))) return rc;
        Fr *coef = (Fr *)ws.poly.ptr, *wdev = coef + head, *l = wdev + wbuf, *h = l + n, *scratch = h + (n - 1);
        HIP_TRY(hipMemcpyAsync(coef, stage.data(), head * sizeof(Fr), hipMemcpyHostToDevice, ws.stream));
        if (w) HIP_TRY(hipMemcpyAsync(wdev, w, n * sizeof(Fr), hipMemcpyHostToDevice, ws.stream));
        const Fr *wsrc = w ? wdev : (const Fr *)d_w;
        if ((rc = FF::combine(ws.stream, p, in, (const uint64_t *)(coef + k + 2), coef, wsrc, l))) return rc;
        // L(z) = 0 for true claimed values; the quotient does not depend on the remainder either way
        if (n > 1 && (rc = PF::suffix(ws.stream, PF::powers_of(z), l, n, h, nullptr, scratch, lanes))) return rc;
        const typename G::J j = commit_or_infinity(ctx, ws, h, n - 1, resident, &rc);
        if (rc) return rc;
        HIP_TRY(hipStreamSynchronize(ws.stream));  // `stage` is pageable host memory: alive until here
        memcpy(out_jac, &j, sizeof j);
        return GMSM_OK;
    }
    // ---- ToLagrangeG1 (gmsm_group_fft.h)
    static int to_lagrange(Context &ctx, const uint64_t *coeffs, const void *d_coeffs, const ResidentBases *from, unsigned log2n,
                           hipStream_t caller, uint64_t *out_affine, void *d_out_affine, ResidentBases *out_bases) {
        GMSM_LEASE_OR_FAIL(lease, ctx);
        Workspace &ws = *lease.w;
        const size_t n = (size_t)1 << log2n, bytes = n * G::AFF_BYTES;
        const void *src;  // host coefficients, else the registered bases, else the device vector
        int rc = stage_input(ws, ws.h2d_points, coeffs, from ? (const void *)from->upoints.ptr : d_coeffs, bytes, {After::NOTHING}, &src);
        if (rc) return rc;
        if ((d_coeffs || d_out_affine) && (rc = order_after(ws, caller))) return rc;  // the caller's stream owns those vectors
        void *dst = d_out_affine;
        if (!dst) {  // host output or a new registration: staged in h2d_points (the load has read any host input by then)
            if ((rc = ws.h2d_points.ensure(bytes))) return rc;
            dst = ws.h2d_points.ptr;
        }
        if ((rc = G::to_lagrange(ws, src, from != nullptr, log2n, dst))) return rc;
        if (out_affine) HIP_TRY(hipMemcpyAsync(out_affine, dst, bytes, hipMemcpyDeviceToHost, ws.stream));
        if (out_bases && (rc = G::register_bases(ctx, dst, n, ws.stream, out_bases))) return rc;
        HIP_TRY(hipStreamSynchronize(ws.stream));
        return GMSM_OK;
    }
    // ---- mpcsetup updates (gmsm_scale.h)
    static int batch_scale(Context &ctx, const uint64_t *points, const void *d_points, size_t n, const uint64_t *scalars, const void *d_scalars,
                           size_t n_scalars, const uint64_t *r, hipStream_t caller, uint64_t *out_affine, void *d_out_affine) {
        GMSM_LEASE_OR_FAIL(lease, ctx);
        Workspace &ws = *lease.w;
        const size_t bytes = n * G::AFF_BYTES;
        const void *src, *dsc;
        int rc = stage_input(ws, ws.h2d_points, points, d_points, bytes, {After::NOTHING}, &src);
        if (rc || (rc = stage_input(ws, ws.h2d_scalars, scalars, d_scalars, n_scalars * sizeof(Fr), {After::NOTHING}, &dsc))) return rc;
        if ((d_points || d_scalars || d_out_affine) && (rc = order_after(ws, caller))) return rc;  // the caller's stream owns those vectors
        void *dst = d_out_affine;
        if (!dst) {  // host output: staged in h2d_points (the kernels have read any host input by the time it is written)
            if ((rc = ws.h2d_points.ensure(bytes))) return rc;
            dst = ws.h2d_points.ptr;
        }
        Fr rr;
        if (r) memcpy(&rr, r, sizeof rr);
        if ((rc = G::batch_scale(ws, src, n, dsc, n_scalars == 1, r ? &rr : nullptr, dst))) return rc;
        if (out_affine) HIP_TRY(hipMemcpyAsync(out_affine, dst, bytes, hipMemcpyDeviceToHost, ws.stream));
        HIP_TRY(hipStreamSynchronize(ws.stream));
        return GMSM_OK;
    }
    static int linear_combinations(Context &ctx, const uint64_t *points, const void *d_points, size_t n, const size_t *ends, size_t n_ends,
                                   const uint64_t *r, hipStream_t caller, uint64_t *out_truncated_jac, uint64_t *out_shifted_jac) {
        GMSM_LEASE_OR_FAIL(lease, ctx);
        Workspace &ws = *lease.w;
        const void *src;
        int rc = stage_input(ws, ws.h2d_points, points, d_points, n * G::AFF_BYTES, {After::STREAM, caller}, &src);
        if (rc) return rc;
        Fr rr;
        memcpy(&rr, r, sizeof rr);
        typename G::J t, s;
        if ((rc = G::linear_combinations(ctx, ws, src, n, ends, n_ends, rr, &t, &s))) return rc;
        HIP_TRY(hipStreamSynchronize(ws.stream));
        memcpy(out_truncated_jac, &t, sizeof t);
        memcpy(out_shifted_jac, &s, sizeof s);
        return GMSM_OK;
    }
    // ---- fr.BatchInvert and the iop ratio polynomials (gmsm_ratio.h); in the G1 tables only: the scalar field is the pair's
    using RF = RatioField<typename G::FrP>;
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
    // holds a call's pageable staging vectors until its stream has drained, whichever way the call leaves
    struct DrainOnExit {
        hipStream_t s;
        ~DrainOnExit() { (void)hipStreamSynchronize(s); }
    };
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
            hipLaunchKernelGGL((k_ratio_publish<typename G::FrP>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const Fr *)z, (Fr *)d_out, n, bad);
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
        Fr bt, gm;
        memcpy(&bt, beta, sizeof bt);
        memcpy(&gm, gamma, sizeof gm);
        std::vector<Fr> table(m);
        RF::coset_table(d, bt, m, table.data());
        const unsigned long long none = ~0ull;
        unsigned long long first_bad = none;
        DrainOnExit drain{ws.stream};
        HIP_TRY(hipMemcpyAsync(bg, table.data(), m * sizeof(Fr), hipMemcpyHostToDevice, ws.stream));
        HIP_TRY(hipMemcpyAsync(lay, layouts, m * sizeof(uint32_t), hipMemcpyHostToDevice, ws.stream));
        HIP_TRY(hipMemcpyAsync(bad, &none, sizeof none, hipMemcpyHostToDevice, ws.stream));
        ratio_settle_events(ws);
        StageTimer timer(ws, true);
        timer.mark(T_DECOMPOSE, ws.stream);
        hipLaunchKernelGGL((k_ratio_factors_copy<typename G::FrP>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ws.stream, in,
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
        Fr bt;
        memcpy(&bt, beta, sizeof bt);
        DrainOnExit drain{ws.stream};
        HIP_TRY(hipMemcpyAsync(lay, num_layouts, m * sizeof(uint32_t), hipMemcpyHostToDevice, ws.stream));
        HIP_TRY(hipMemcpyAsync(lay + m, den_layouts, m * sizeof(uint32_t), hipMemcpyHostToDevice, ws.stream));
        ratio_settle_events(ws);
        StageTimer timer(ws, true);
        timer.mark(T_DECOMPOSE, ws.stream);
        hipLaunchKernelGGL((k_ratio_factors_shuffled<typename G::FrP>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ws.stream, pn,
                           (const Fr *)pd, (const uint32_t *)lay, m, n, d->log2n, bt, b.fnum, b.fden);
        HIP_TRY(hipGetLastError());
        return ratio_finish(ws, timer, d, b, n, basis, layout, out, d_out, nullptr, nullptr);
    }
    // ---- iop.Polynomial: basis changes, Evaluate, DivideByXMinusOne (gmsm_iop_poly.h); in the G1 tables only, like the ratios
    using IP = IopPolyField<typename G::FrP>;
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
            const FftPowers<typename G::FrP> pw = FftField<typename G::FrP>::powers_of(xx);
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
    // ---- iop.Evaluate of a straight-line program (gmsm_iop_expr.h); in the G1 tables only. ws.poly holds the result of a
    // host-output call, then the call's small tables in one piece: the constants, the input descriptors, the program.
    using IE = IopExprField<typename G::FrP>;
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
    // ---- fr/polynomial.MultiLin and one GKR sumcheck claim (gmsm_gkr.h); in the G1 tables only
    using GK = GkrField<typename G::FrP>;
    static constexpr auto multilin_fold = &GK::multilin_fold;
    static constexpr auto multilin_evaluate = &GK::multilin_evaluate;
    static constexpr auto multilin_eq = &GK::multilin_eq;
    static constexpr auto gkr_new = &GK::gkr_new;
    static constexpr auto gkr_next = &GK::gkr_next;
    static constexpr auto gkr_final = &GK::gkr_final;
    static const GroupVTable *get() {
        // Filled by name: several members have the same type (decode_raw / decode_compressed, fold / jac_to_affine), so a
        // positional list with two of them swapped would compile.
        static const GroupVTable vt = [] {
            GroupVTable v{};
            v.fr_bits = G::FR_BITS, v.fr_max_order = (unsigned)G::FrP::MAX_ORDER;
            v.aff_bytes = G::AFF_BYTES, v.scalar_bytes = G::SCALAR_BYTES, v.jac_bytes = sizeof(typename G::J), v.xyzz_bytes = sizeof(typename G::Ext);
#define GMSM_VT(f) v.f = &f
            // In the order of the struct's members: the kernels of a group's code object are instantiated in the order their
            // callers are first named here, so this order decides the object's layout.
            GMSM_VT(multiexp_host), GMSM_VT(multiexp_device), GMSM_VT(window_sums), GMSM_VT(fold), GMSM_VT(jac_to_affine);
            GMSM_VT(debug_decompose), GMSM_VT(debug_field_op), GMSM_VT(debug_group_op), GMSM_VT(generate_points);
            GMSM_VT(register_bases), GMSM_VT(submit), GMSM_VT(collect), GMSM_VT(window_sums_enqueue), GMSM_VT(fold_sets), GMSM_VT(fold_powers);
            GMSM_VT(multiexp_bases_host), GMSM_VT(batch_scalar_mul), GMSM_VT(batch_jac_to_affine);
            GMSM_VT(decode_raw), GMSM_VT(validate_points), GMSM_VT(decode_compressed), GMSM_VT(encode_compressed);
            GMSM_VT(fft_domain_new), GMSM_VT(fft_run), GMSM_VT(fft_bit_reverse);
            GMSM_VT(precompute_tables), GMSM_VT(tables_serve), GMSM_VT(shard_piece), GMSM_VT(host_piece_ranges);
            GMSM_VT(debug_glv_split), GMSM_VT(plan_info), GMSM_VT(reduce_shape), GMSM_VT(run_layout), GMSM_VT(fold_planes);
            GMSM_VT(poly_eval), GMSM_VT(poly_div), GMSM_VT(kzg_open);
            if constexpr (IS_G1) GMSM_VT(to_lagrange);  // the three G1-only members stay null for the G2 groups
            GMSM_VT(fflonk_next_divisor), GMSM_VT(open_check), GMSM_VT(fflonk_fold);
            if constexpr (IS_G1) GMSM_VT(open_w), GMSM_VT(open_wprime);
            GMSM_VT(batch_scale), GMSM_VT(linear_combinations);
            if constexpr (IS_G1) GMSM_VT(fr_batch_invert), GMSM_VT(ratio_copy), GMSM_VT(ratio_shuffled);
            if constexpr (IS_G1) GMSM_VT(iop_to_basis), GMSM_VT(iop_evaluate), GMSM_VT(iop_quotient);
            if constexpr (IS_G1) GMSM_VT(iop_expr);
            if constexpr (IS_G1)
                v.multilin_fold = multilin_fold, v.multilin_evaluate = multilin_evaluate, v.multilin_eq = multilin_eq, v.gkr_new = gkr_new,
                v.gkr_next = gkr_next, v.gkr_final = gkr_final;
#undef GMSM_VT
            return v;
        }();
        return &vt;
    }
};

}  // namespace gmsm
