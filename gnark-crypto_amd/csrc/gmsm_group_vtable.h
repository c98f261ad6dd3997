// The function table of one (curve, group): what the C ABI (gmsm_engine.hip) dispatches through - argument marshalling
// between the ABI's uint64_t limbs / void pointers and the typed entry points of struct Group. Included by gmsm_group.h.
// What is over the scalar field alone has a table of its own (gmsm_field_vtable.h).
#pragma once
#include "gmsm_group.h"
#include "gmsm_group_debug.h"
#include "gmsm_field_vtable.h"

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
    // ---- KZG opening (gmsm_poly.h); the polynomials are staged as the scalar field's own entries stage them
    using FV = FieldVTableOf<typename G::FrP>;
    using PF = PolyField<typename G::FrP>;
    using Fr = Fp<typename G::FrP>;
    static_assert(sizeof(Fr) == G::SCALAR_BYTES, "fr.Element layout");
    static int kzg_open(Context &ctx, const uint64_t *polys, const void *d_polys, const size_t *lens, size_t k, const uint64_t *point,
                        const uint64_t *gamma, hipStream_t caller, uint64_t *out_claimed, uint64_t *out_jac, const ResidentBases *resident) {
        GMSM_LEASE_OR_FAIL(lease, ctx);
        Workspace &ws = *lease.w;
        size_t total = 0, maxlen = 0;
        for (size_t i = 0; i < k; ++i) total += lens[i], maxlen = std::max(maxlen, lens[i]);
        const Fr *in;
        int rc = FV::poly_input(ws, polys, d_polys, total, caller, &in);
        if (rc) return rc;
        const bool folds = k > 1;
        const size_t ol_elems = folds ? FV::word_slots(2 * k) : 0;
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
    static int fflonk_fold(Context &ctx, const uint64_t *polys, const void *d_polys, const size_t *lens, size_t npolys, hipStream_t caller,
                           uint64_t *out, void *d_out, const ResidentBases *resident, uint64_t *out_jac) {
        typename FF::Plan p;
        int rc = FF::plan("gmsm_fflonk_fold", lens, &npolys, 1, nullptr, nullptr, false, 0, &p);
        if (rc) return rc;
        GMSM_LEASE_OR_FAIL(lease, ctx);
        Workspace &ws = *lease.w;
        const Fr *in;
        if ((rc = FV::poly_input(ws, polys, d_polys, p.total, caller, &in))) return rc;
        if (d_out && polys && (rc = order_after(ws, caller))) return rc;  // the caller's stream may still use d_out
        const size_t head = FV::word_slots(p.table_words()), fbuf = d_out ? 0 : p.maxfold;
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
        if ((rc = FV::poly_input(ws, polys, d_polys, p.total, caller, &in))) return rc;
        if (d_out_w && polys && (rc = order_after(ws, caller))) return rc;  // the caller's stream may still use d_out_w
        const size_t wbuf = out_w ? p.maxfold : 0, ping = p.maxmember - 1;
        const unsigned lanes = PF::lane_option();
        const size_t scratch_elems = SF::chain_scratch(lens, p.member_points.data(), p.npolys, lanes);
        if ((rc = ws.poly.ensure((p.nrem + wbuf + 2 * ping + scratch_elems) * sizeof(Fr)))) return rc;
        Fr *rem = (Fr *)ws.poly.ptr, *w = out_w ? rem + p.nrem : (Fr *)d_out_w, *a = rem + p.nrem + wbuf, *b = a + ping, *scratch = b + ping;
        if ((rc = FF::chains(ws.stream, p, in, lens, fr_from_limbs<Fr>(gamma), rem, w, a, b, scratch, lanes))) return rc;
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
        if ((rc = FV::poly_input(ws, polys, d_polys, p.total, caller, &in))) return rc;
        if (d_w && polys && (rc = order_after(ws, caller))) return rc;  // d_w is the caller's stream's
        // host part: shplonk's c_i, Z_T(z), sum_i c_i r_i(z) over the extended sets and the inner claimed values (singleton
        // form: the sets and the claimed values as given), then the index tables, in one staging vector of Fr-sized slots
        const size_t head = k + 2 + FV::word_slots(p.table_words());
        std::vector<Fr> stage(head);
        SF::combine_coefficients(p.ext.data(), p.ext_npoints.data(), k, (const Fr *)folded_claimed, fr_from_limbs<Fr>(gamma), fr_from_limbs<Fr>(z),
                                 stage.data());
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
        if (r) rr = fr_from_limbs<Fr>(r);
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
        typename G::J t, s;
        if ((rc = G::linear_combinations(ctx, ws, src, n, ends, n_ends, fr_from_limbs<Fr>(r), &t, &s))) return rc;
        HIP_TRY(hipStreamSynchronize(ws.stream));
        memcpy(out_truncated_jac, &t, sizeof t);
        memcpy(out_shifted_jac, &s, sizeof s);
        return GMSM_OK;
    }
    static const GroupVTable *get() {
        // Filled by name: several members have the same type (decode_raw / decode_compressed, fold / jac_to_affine), so a
        // positional list with two of them swapped would compile.
        static const GroupVTable vt = [] {
            GroupVTable v{};
            v.fr_bits = G::FR_BITS;
            v.aff_bytes = G::AFF_BYTES, v.scalar_bytes = G::SCALAR_BYTES, v.jac_bytes = sizeof(typename G::J), v.xyzz_bytes = sizeof(typename G::Ext);
#define GMSM_VT(f) v.f = &f
            // In the order of the struct's members: the kernels of a group's code object are instantiated in the order their
            // callers are first named here, so this order decides the object's layout.
            GMSM_VT(multiexp_host), GMSM_VT(multiexp_device), GMSM_VT(window_sums), GMSM_VT(fold), GMSM_VT(jac_to_affine);
            GMSM_VT(debug_decompose), GMSM_VT(debug_field_op), GMSM_VT(debug_group_op), GMSM_VT(generate_points);
            GMSM_VT(register_bases), GMSM_VT(submit), GMSM_VT(collect), GMSM_VT(window_sums_enqueue), GMSM_VT(fold_sets), GMSM_VT(fold_powers);
            GMSM_VT(multiexp_bases_host), GMSM_VT(batch_scalar_mul), GMSM_VT(batch_jac_to_affine);
            GMSM_VT(decode_raw), GMSM_VT(validate_points), GMSM_VT(decode_compressed), GMSM_VT(encode_compressed);
            GMSM_VT(precompute_tables), GMSM_VT(tables_serve), GMSM_VT(shard_piece), GMSM_VT(host_piece_ranges);
            GMSM_VT(debug_glv_split), GMSM_VT(plan_info), GMSM_VT(reduce_shape), GMSM_VT(run_layout), GMSM_VT(fold_planes);
            GMSM_VT(kzg_open);
            if constexpr (IS_G1) GMSM_VT(to_lagrange);  // the three G1-only members stay null for the G2 groups
            GMSM_VT(fflonk_fold);
            if constexpr (IS_G1) GMSM_VT(open_w), GMSM_VT(open_wprime);
            GMSM_VT(batch_scale), GMSM_VT(linear_combinations);
#undef GMSM_VT
            return v;
        }();
        return &vt;
    }
};

}  // namespace gmsm
