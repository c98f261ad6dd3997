/* gmsm.h -- C ABI of the MI355X multi-scalar-multiplication engine (libgmsm.so).
 *
 * Drop-in boundary for gnark-crypto's  (*G1Jac).MultiExp / (*G2Jac).MultiExp
 *   ecc/bn254/multiexp.go:32 (G1) and :357 (G2); ecc/bls12-381/multiexp.go:32,:355; ecc/bw6-761/multiexp.go:32,:306
 * A build-tagged Go file per curve package replaces the body of those methods (after the two argument checks,
 * multiexp.go:61-71) with one cgo call to the matching symbol below; (*G1Affine).MultiExp, Fold, kzg.Commit,
 * pedersen etc. route through it unchanged.  INTEGRATION.md shows the cgo stub.
 *
 * Memory layout (identical to the Go slices, so `unsafe.Pointer(&points[0])` is passed without copying):
 *   points   n x {X,Y}           each coordinate = fp.Element  = FP_LIMBS little-endian uint64, Montgomery form;
 *                                G2 over Fp2: X.A0, X.A1, Y.A0, Y.A1.  The affine point (0,0) is infinity.
 *   scalars  n x fr.Element      FR_LIMBS little-endian uint64, Montgomery form.
 *   out_jac  {X,Y,Z}             Jacobian, Montgomery form; Z = 0 (X = Y = 1) for infinity.  Any representative of
 *                                the group element (as in the reference, callers compare with Equal or FromJacobian).
 *   curve      FP_LIMBS FR_LIMBS   G1Affine  G2Affine  (bytes)
 *   bn254         4        4          64       128
 *   bls12_381     6        4          96       192
 *   bw6_761      12        6         192       192     (G2 is over Fp)
 *
 * Return codes:  GMSM_OK, GMSM_ERR_LEN  ("len(points) != len(scalars)", multiexp.go:63),
 *                GMSM_ERR_CONFIG ("invalid config: config.NbTasks > 1024", multiexp.go:70),
 *                >= GMSM_ERR_DEVICE: HIP/runtime failure -- gmsm_last_error() has the text.  There is NO CPU
 *                fallback inside this library: without a usable gfx950 device every compute entry fails loudly.
 *
 * Threading: every entry point is re-entrant and may be called concurrently from any OS thread (goroutines
 * migrate); per device up to three calls run at a time (three workspaces, of which submitted tickets hold at most two, so a
 * blocking entry never waits for somebody else's gmsm_multiexp_collect), further callers wait their turn.
 * Several GPUs: OPT-IN. A process that configures nothing runs every drop-in call on one device (gmsm_set_device, else
 * device 0) and touches no other - the usual deployment is one prover per GPU. After gmsm_set_devices(list) or with
 * GMSM_DEVICES="0,1,2,3" / "all" in the environment (read once) the drop-in entries spread every MultiExp of 2^17 points
 * or more over the listed devices (point slices, one host thread per device, one fold; see gmsm_multiexp_sharded); the
 * footprint is then one context per listed device: six streams, pinned result buffers, scratch that grows with the
 * largest call (gmsm_trim gives it back) and two pooled host threads.
 * Limits: n < 2^31. One pipeline run takes up to 2^27 points; the MultiExp entries split larger inputs into point
 * ranges themselves, gmsm_window_sums_* and gmsm_multiexp_bases_submit refuse them (GMSM_ERR_ARG).
 * Ownership: the caller owns all buffers; host pointers are not retained after return.
 */
#ifndef GMSM_H
#define GMSM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GMSM_OK 0
#define GMSM_ERR_LEN 1
#define GMSM_ERR_CONFIG 2
#define GMSM_ERR_DEVICE 3
#define GMSM_ERR_ARG 4
#define GMSM_ERR_POINT 5 /* a point failed decoding / validation; *bad_index has its position, gmsm_last_error() why */

/* group ids for the generic entry points */
enum gmsm_group {
    GMSM_BN254_G1 = 0,
    GMSM_BN254_G2 = 1,
    GMSM_BLS12_381_G1 = 2,
    GMSM_BLS12_381_G2 = 3,
    GMSM_BW6_761_G1 = 4,
    GMSM_BW6_761_G2 = 5,
    GMSM_NUM_GROUPS = 6
};

/* ---- drop-in entries: host pointers in, Jacobian out (replaces (*GxJac).MultiExp after its argument checks;
 *      the checks are repeated here so that the error behaviour is identical when called directly). ---- */
int gmsm_bn254_g1_multiexp(const uint64_t *points, size_t n_points, const uint64_t *scalars, size_t n_scalars,
                           int nb_tasks, uint64_t *out_jac); /* ecc/bn254/multiexp.go:32 */
int gmsm_bn254_g2_multiexp(const uint64_t *points, size_t n_points, const uint64_t *scalars, size_t n_scalars,
                           int nb_tasks, uint64_t *out_jac); /* ecc/bn254/multiexp.go:357 */
int gmsm_bls12_381_g1_multiexp(const uint64_t *points, size_t n_points, const uint64_t *scalars, size_t n_scalars,
                               int nb_tasks, uint64_t *out_jac); /* ecc/bls12-381/multiexp.go:32 */
int gmsm_bls12_381_g2_multiexp(const uint64_t *points, size_t n_points, const uint64_t *scalars, size_t n_scalars,
                               int nb_tasks, uint64_t *out_jac); /* ecc/bls12-381/multiexp.go:355 */
int gmsm_bw6_761_g1_multiexp(const uint64_t *points, size_t n_points, const uint64_t *scalars, size_t n_scalars,
                             int nb_tasks, uint64_t *out_jac); /* ecc/bw6-761/multiexp.go:32 */
int gmsm_bw6_761_g2_multiexp(const uint64_t *points, size_t n_points, const uint64_t *scalars, size_t n_scalars,
                             int nb_tasks, uint64_t *out_jac); /* ecc/bw6-761/multiexp.go:306 */

/* Same, selected by id. */
int gmsm_multiexp(int group, const uint64_t *points, size_t n_points, const uint64_t *scalars, size_t n_scalars,
                  int nb_tasks, uint64_t *out_jac);

/* (*GxAffine).MultiExp (multiexp.go:20-27): MultiExp followed by FromJacobian (g1.go:150-166); out_affine = {X,Y},
 * (0,0) for infinity.  This is the canonical value parity is defined on. */
int gmsm_multiexp_affine(int group, const uint64_t *points, size_t n_points, const uint64_t *scalars,
                         size_t n_scalars, int nb_tasks, uint64_t *out_affine);

/* (*G1Jac).Fold / (*G2Jac).Fold (ecc/bn254/multiexp.go:331-340, G2 :657-665): sum_i points[i] * coeff^i. coeff is one
 * fr.Element (Montgomery limbs); the powers are formed on the host exactly as the reference does, then MultiExp. */
int gmsm_fold(int group, const uint64_t *points, size_t n_points, const uint64_t *combination_coeff, int nb_tasks,
              uint64_t *out_jac);

/* ---- one MultiExp over several GPUs of the node, inside the library.  The reference spreads a
 *      MultiExp over the cores of the machine - one worker per c-bit window collected on a channel
 *      (ecc/bn254/multiexp.go:148-209), and a split of the points in two halves whose results are added (:98-140) -; here
 *      the workers are the devices: one host thread per logical rank runs its piece on its device, the ranks' window totals
 *      (<= 64 extended-Jacobian points each) come back through each device's pinned result buffer and the calling thread
 *      runs the one fold (multiexp.go:302-315).  Same arguments, layouts, return codes and result as gmsm_multiexp.
 *      devices / n_devices: one entry per logical rank, a device may appear more than once (ranks on one device share
 *      its workspaces); NULL / 0 = the configured list (gmsm_set_devices, else GMSM_DEVICES), and every visible device
 *      when nothing is configured - this entry is an explicit request for several devices.  mode: 0 auto (= 1), 1 points - rank r takes points [r n/G, (r+1) n/G) and all windows; every device
 *      copies only its slice over its own PCIe link -, 2 windows - rank r takes windows r, r+G, ... of all points (the
 *      reference's per-window workers; every rank needs all bases).  Ranks whose slice would fall below 2^16 points are
 *      left out.  gmsm_<curve>_g{1,2}_multiexp, gmsm_multiexp, gmsm_multiexp_affine and gmsm_fold call this themselves
 *      when more than one device has been configured (opt-in, see "Several GPUs" above).  Every worker checks that it runs
 *      on the device of its context; a failure names the rank and the device. ---- */
int gmsm_multiexp_sharded(int group, const uint64_t *points, size_t n_points, const uint64_t *scalars, size_t n_scalars,
                          int nb_tasks, const int *devices, int n_devices, int mode, uint64_t *out_jac);
/* Resident bases on several devices: the n bases are uploaded (all devices at once, each over its own link) and
 * rewritten once on every distinct device of the list - full copies, so that any prefix can be cut evenly over the ranks.
 * The handle is accepted by gmsm_multiexp_bases (host scalars; sharded like gmsm_multiexp_sharded, mode auto),
 * gmsm_multiexp_bases_sharded (explicit mode), gmsm_multiexp_bases_batch (host scalars: the k vectors are independent
 * MultiExp calls, rank r runs the block [r k/G, (r+1) k/G) of them on its device's copy - no sharding of a single call and
 * no exchange; kzg.Commit per polynomial, ecc/bn254/kzg/kzg.go:159-176) and gmsm_bases_release; the device-pointer
 * entries take single-device handles only. */
int gmsm_bases_register_sharded(int group, const uint64_t *points, size_t n, const int *devices, int n_devices,
                                uint64_t *out_handle);
int gmsm_multiexp_bases_sharded(uint64_t handle, const uint64_t *scalars, size_t n_scalars, int nb_tasks, int mode,
                                uint64_t *out_jac);
/* Window tables for registered bases (any handle of gmsm_bases_register* / _sharded): the multiples 2^(c w) P_i of every
 * base for every window w of the c-bit decomposition are computed once and kept in HBM (nwin copies of the bases: BN254 G1,
 * 2^20 bases, c = 19: 14 x 64 MiB - sized for 288 GB).  Every later MultiExp over the handle (all gmsm_multiexp_bases*
 * entries, tickets, batches, point-sharded calls) then drops the digits of ALL windows into ONE set of 2^(c-1) buckets:
 * one bucket reduction instead of nwin, and a wider window (fewer additions) than the plain path can afford.  Same
 * group element, hence the same affine result, as without tables (the reference has no counterpart: its MultiExp takes
 * the bases anew on every call, ecc/bn254/multiexp.go:61; this is what kzg.Commit over a fixed SRS can use,
 * ecc/bn254/kzg/kzg.go:159-176).  c = 0: the library's width for this many bases; 2..20 otherwise.  Calls over a prefix
 * shorter than n/16, call sizes outside the range where the tables were measured to win (about 2^13..2^21 points, by
 * group) and calls with GMSM_OPT_WINDOW_BITS forced to another width use the plain path; GMSM_OPT_TABLES = 0 switches the
 * tables off, 2 uses them for every call size (tests).
 * The same call also builds NARROW tables (width 6) over the first 4096 bases (2048 for BW6-761): a MultiExp of at most that many points over the
 * handle (Pedersen commitments, small KZG commitments over a fixed SRS) then runs the fused small-n kernel with one bucket
 * set per workgroup and needs no host-side fold of window totals at all - BN254 G1, 2^10 points: 0.146 ms against 0.181 ms
 * for the same call without tables.
 * Safe while other threads use the handle: the tables are published (release store of their width) only when complete,
 * calls that started earlier keep the plain path; concurrent precompute calls on one handle are serialised.  Bases outside the prime-order subgroup whose multiples reach
 * the identity are refused (GMSM_ERR_ARG; the handle keeps working without tables).
 * gmsm_bases_table_bits: the width of the handle's tables, 0 = none. */
int gmsm_bases_precompute(uint64_t handle, unsigned c);
unsigned gmsm_bases_table_bits(uint64_t handle);
unsigned long gmsm_debug_table_runs(void); /* pipeline runs that went through window tables so far (tests) */
unsigned long gmsm_debug_small_runs(void); /* calls served by the fused small-n kernel so far (tests) */
/* The devices the drop-in entries shard over (one entry per logical rank); count = 0 restores the default (GMSM_DEVICES
 * if set, else no spreading: one device).  gmsm_get_devices returns the number of configured ranks (1 and the calling
 * thread's device when nothing is configured; -1 when GMSM_DEVICES is malformed) and writes up to max_devices of them
 * (out_devices may be NULL). */
int gmsm_set_devices(const int *devices, int count);
int gmsm_get_devices(int *out_devices, int max_devices);

/* ---- device-resident entries (bases/scalars already in HBM: the SRS-resident fast path).
 *      d_points / d_scalars are device pointers with the layouts above; hip_stream is the hipStream_t the inputs were
 *      produced on (NULL = default stream): the engine runs on a private stream ordered after the work queued there;
 *      the call returns after the result has been copied back to out_jac (host memory).
 *      Concurrency (all blocking entries): any number of threads may call at once; per device up to three calls are in
 *      flight at a time, each on its own workspace and streams - the sort and accumulation of one overlap the
 *      latency-bound reduction, copy-back and host fold of another - and further callers wait their turn. At most two of
 *      the three workspaces are ever held by uncollected tickets (gmsm_multiexp_submit), so a blocking call never waits
 *      for somebody else's gmsm_multiexp_collect. ---- */
int gmsm_multiexp_device(int group, const void *d_points, const void *d_scalars, size_t n, void *hip_stream,
                         uint64_t *out_jac);

/* ---- resident bases (device-resident SRS): the bases of e.g. a KZG proving key
 *      (ecc/bn254/kzg/kzg.go:35-37) are uploaded and rewritten into the engine's internal form once;
 *      every later MultiExp over a prefix of them (kzg.Commit: pk.G1[:len(p)], kzg.go:159-176) sends only scalars.
 *      Give exactly one of `points` (host, Go layout) / `d_points` (device, Go layout). ---- */
int gmsm_bases_register(int group, const uint64_t *points, const void *d_points, size_t n, uint64_t *out_handle);
int gmsm_bases_release(uint64_t handle);
/* scalars on the host (n_scalars <= registered n) */
int gmsm_multiexp_bases(uint64_t handle, const uint64_t *scalars, size_t n_scalars, int nb_tasks, uint64_t *out_jac);
/* scalars already on the device */
int gmsm_multiexp_bases_device(uint64_t handle, const void *d_scalars, size_t n_scalars, void *hip_stream,
                               uint64_t *out_jac);

/* ---- two MultiExp calls in flight (the reference's equivalent is several goroutines calling
 *      MultiExp at once, BenchmarkManyMultiExpG1Reference, ecc/bn254/multiexp_test.go:385-415).
 *      submit launches the whole device pipeline for device-resident scalars over registered bases and returns without
 *      waiting for the device; collect waits, folds the windows and writes the Jacobian result. At most two tickets may be
 *      outstanding per device: a third submit returns GMSM_ERR_ARG at once. A device has three workspaces; when all of
 *      them are leased at that moment (blocking callers in other threads, gmsm_trim) submit waits for the first to be
 *      released, as a blocking entry would - that wait always ends, because tickets never hold more than two of the
 *      three. A caller still waiting when gmsm_shutdown runs gets GMSM_ERR_DEVICE. d_scalars must stay valid until its
 *      ticket is collected.
 *      hip_stream: the stream the scalars were produced on (NULL = the default stream); the pipeline is ordered
 *      after the work already queued there. The sort/accumulate of one call overlaps the latency-bound bucket reduction, copy-back and
 *      host fold of the other. ---- */
int gmsm_multiexp_bases_submit(uint64_t handle, const void *d_scalars, size_t n_scalars, void *hip_stream,
                               uint64_t *out_ticket);
int gmsm_multiexp_collect(uint64_t ticket, uint64_t *out_jac);
/* (a ticket takes at most 2^27 points, and so does every vector of gmsm_multiexp_bases_batch below: submit refuses more
 * with GMSM_ERR_ARG; the blocking single-vector entries split larger inputs themselves)
 * k MultiExp over the same registered bases in one blocking call (one commitment per polynomial with a fixed SRS:
 * kzg.Commit, ecc/bn254/kzg/kzg.go:159-176; BatchOpenSinglePoint :246): scalars = k x n fr.Element, contiguous, either on
 * the host (`scalars`) or on the device (`d_scalars`, produced on hip_stream); out_jac = k Jacobian results. Two of
 * the k calls are in flight at a time; host scalars of vector i+1 are copied while vector i is being accumulated. */
int gmsm_multiexp_bases_batch(uint64_t handle, const uint64_t *scalars, const void *d_scalars, size_t n, size_t k,
                              void *hip_stream, uint64_t *out_jac);

/* ---- fixed-base batch: BatchScalarMultiplicationG1/G2 (ecc/bn254/g1.go:1039-1118; the step that
 *      builds an SRS, kzg.NewSRS) and BatchJacobianToAffineG1 (g1.go:989-1035). out[i] = scalars[i] * base in affine
 *      coordinates (unique, so results are bit-comparable); scalars are Montgomery fr.Element as everywhere else.
 *      On the device every scalar costs nwin mixed additions from a table of all windows' multiples (no doublings), then
 *      one shared inversion per 32 results. The _device variant reads d_scalars (produced on hip_stream) and writes
 *      n Go-layout affine points to d_out_affine; it returns when they are complete. ---- */
int gmsm_batch_scalar_mul(int group, const uint64_t *base_affine, const uint64_t *scalars, size_t n, uint64_t *out_affine);
int gmsm_batch_scalar_mul_device(int group, const uint64_t *base_affine, const void *d_scalars, size_t n, void *hip_stream,
                                 void *d_out_affine);
/* jac = n x {X, Y, Z} (Go G1Jac/G2Jac layout), Z = 0 -> (0, 0) */
int gmsm_batch_jac_to_affine(int group, const uint64_t *jac, size_t n, uint64_t *out_affine);

/* ---- point ingest: the step before the MSM - points arrive as bytes and must become validated
 *      Montgomery limbs in HBM.  `check`: 0 decode only, 1 + on the curve, 2 + in the r-torsion (the Decoder's default,
 *      ecc/bn254/marshal.go:250-275), decided by the reference's own endomorphism identities (IsInSubGroup:
 *      ecc/bls12-381/g1.go:481-492, g2.go:484-491, ecc/bn254/g2.go:483-497, ecc/bw6-761/g1.go:482-496), 3 = the same
 *      predicate decided as the definition says, "on the curve and [r]P = infinity" (2-6 x the group operations; the
 *      cross-check of level 2).  On a bad point the call returns GMSM_ERR_POINT,
 *      *bad_index is the first offender and gmsm_last_error() carries the reference's error text; otherwise *bad_index = -1.
 *
 *      gmsm_points_from_raw: raw = n points in the uncompressed wire format of (*G1Affine).RawBytes() /
 *      Encoder(RawEncoding()) (marshal.go:826, G2 :1078; bls12-381/marshal.go:855): big-endian, regular (non-Montgomery)
 *      form, X | Y (Fp2: A1 | A0), metadata in the top bits of the first byte, n * gmsm_affine_limbs(group) * 8 bytes in
 *      total.  Compressed encodings are refused here (gmsm_points_from_compressed below).  Decoded points go to out_affine (host) and/or d_out_affine (device);
 *      give at least one.
 *      gmsm_points_validate: the same checks over points that are already Go-layout limbs (host or device).
 *      gmsm_bases_register_raw: decode + check + register in one call (the SRS never exists on the host in limb form).
 *      gmsm_bases_register_dump: an SRS dump written by kzg.SRS.WriteDump (ecc/bn254/kzg/marshal.go:65-95) ends in
 *      unsafe.WriteMarker + unsafe.WriteSlice(pk.G1) = u64 0xdeadbeef | u64 length | raw []G1Affine memory
 *      (utils/unsafe/dump_slice.go:16-32, :80).  `offset` is the byte position of the marker (expect_marker != 0) or of
 *      the length word; at most max_points (0 = all) are loaded, like ReadDump's maxPkPoints.  The file is streamed
 *      through pinned buffers straight into HBM and registered; *out_n receives the number of bases.  ReadDump validates
 *      nothing; check > 0 runs the validation kernel over the loaded points. ---- */
int gmsm_points_from_raw(int group, const uint8_t *raw, size_t n, int check, uint64_t *out_affine, void *d_out_affine,
                         int64_t *bad_index);
int gmsm_points_validate(int group, const uint64_t *points, const void *d_points, size_t n, int check, int64_t *bad_index);
int gmsm_bases_register_raw(int group, const uint8_t *raw, size_t n, int check, uint64_t *out_handle, int64_t *bad_index);
/* The Encoder's DEFAULT format - compressed points, what (*G1Affine).Bytes() writes and kzg.SRS.WriteTo / ReadFrom move
 * (ecc/bn254/marshal.go:801-823, :907-948; G2 :1051-1075, :1168-1215; bls12-381/marshal.go:25-35 for the 3-bit flags): X only,
 * gmsm_affine_limbs(group) * 4 bytes a point (Fp2: X.A1 | X.A0), the flag bits say which root Y is (LexicographicallyLargest).
 *   gmsm_points_from_compressed: decode (Y = sqrt(X^3 + b) on the device: the compute-heavy half of Decoder.Decode,
 *      unsafeComputeY, marshal.go:951-989) + the checks of `check` (the curve equation holds by construction; 2 / 3 add the
 *      subgroup test).  Errors as the reference words them: "invalid compressed coordinate: square root doesn't exist",
 *      "invalid infinity point encoding", "invalid fp.Element encoding", "invalid point: subgroup check failed"; uncompressed
 *      or undefined flags are refused (gmsm_points_from_raw takes those).
 *   gmsm_points_compress: the encoder, points (host) or d_points (device) -> out_comp (host).
 *   gmsm_bases_register_compressed: decode + check + register in one call. */
int gmsm_points_from_compressed(int group, const uint8_t *comp, size_t n, int check, uint64_t *out_affine, void *d_out_affine,
                                int64_t *bad_index);
int gmsm_points_compress(int group, const uint64_t *points, const void *d_points, size_t n, uint8_t *out_comp);
int gmsm_bases_register_compressed(int group, const uint8_t *comp, size_t n, int check, uint64_t *out_handle, int64_t *bad_index);
int gmsm_bases_register_dump(int group, const char *path, uint64_t offset, int expect_marker, size_t max_points, int check,
                             uint64_t *out_handle, size_t *out_n, int64_t *bad_index);

/* ---- fr/fft: ecc/<curve>/fr/fft on the device, over the scalar field of `group`'s curve (G1 and
 *      G2 ids of a curve name the same field).  gmsm_fft_domain_new = fft.NewDomain(m) (fr/fft/domain.go:66): cardinality
 *      = next power of two >= m, Generator = fr.Generator(m) (fr/generator.go:18-36), coset shift = the generator of Fr^*
 *      (domain.go:56-62; 5 / 7 / 15 for BN254 / BLS12-381 / BW6-761); twiddles live in HBM, coset tables appear with the
 *      first coset transform.  gmsm_fft = (*Domain).FFT (inverse = 0) / FFTInverse (inverse != 0), fft.go:31-196:
 *      decimation 0 = DIT (input bit-reversed, output natural), 1 = DIF (input natural, output bit-reversed);
 *      on_coset = the OnCoset() option.  a: n = cardinality fr.Elements (Montgomery limbs), transformed in place, either on
 *      the host (`a`) or on the device (`d_a`, produced on hip_stream; the call returns when the result is complete).
 *      gmsm_fft_bit_reverse = fft.BitReverse (bitreverse.go:20).  Results are bit-identical to the reference's: every
 *      output is a uniquely determined field element in canonical Montgomery form. ---- */
int gmsm_fft_domain_new(int group, uint64_t m, uint64_t *out_handle);
int gmsm_fft_domain_release(uint64_t handle);
/* Cardinality and the domain's field constants (fr.Element limbs each; any pointer may be NULL) */
int gmsm_fft_domain_info(uint64_t handle, uint64_t *cardinality, uint64_t *generator, uint64_t *generator_inv,
                         uint64_t *cardinality_inv, uint64_t *fr_multiplicative_gen, uint64_t *fr_multiplicative_gen_inv);
int gmsm_fft(uint64_t handle, uint64_t *a, void *d_a, size_t n, int inverse, int decimation, int on_coset, void *hip_stream);
int gmsm_fft_bit_reverse(int group, uint64_t *a, void *d_a, size_t n, void *hip_stream);

/* ---- KZG opening (ecc/<curve>/kzg/kzg.go): the host arithmetic of Open and BatchOpenSinglePoint on the device, over the
 *      scalar field of `group`'s curve; results are bit-identical to the reference's (canonical Montgomery fr.Element).
 *      Polynomials are fr.Element coefficient vectors, lowest degree first; k of them are concatenated (lens[i]
 *      coefficients each), given as exactly one of a host pointer / a device pointer (16-byte aligned, produced on
 *      hip_stream). Inputs are never modified. Every call returns when its results are complete; scratch comes from the
 *      workspace of the call (gmsm_trim gives it back).
 *   gmsm_poly_eval: out_values[i] = f_i(point), Horner (eval, kzg.go:55-63); an empty polynomial is GMSM_ERR_ARG.
 *   gmsm_poly_div_x_minus_a: dividePolyByXminusA (kzg.go:565-583): h = (f - f(a)) / (X - a), n - 1 coefficients to exactly
 *      one of out_h (host) / d_out_h (device), and f(a) to out_value (may be NULL). n == 1: f(a) and an empty quotient;
 *      n == 0 is GMSM_ERR_ARG.
 *   gmsm_kzg_open: kzg.Open over registered bases (gmsm_bases_register*): out_claimed = f(point), out_h_jac =
 *      Commit(dividePolyByXminusA(f)) as Jacobian {X,Y,Z}. The quotient stays in HBM and goes through the resident MultiExp
 *      (window tables included when the handle has them).
 *   gmsm_kzg_open_folded: BatchOpenSinglePoint after the Fiat-Shamir challenge gamma (deriveGamma stays with the caller):
 *      out_h_jac = Commit((sum_i gamma^i f_i - sum_i gamma^i f_i(a)) / (X - a)), f_i zero beyond lens[i] (kzg.go:302-326).
 *   Errors as the reference: n == 0, n == 1 (the empty quotient, which Commit refuses), n > the registered size, and in the
 *   batch entry any empty member or a largest member of length 1, are GMSM_ERR_ARG with the text
 *   "invalid polynomial size (larger than SRS or == 0)". ---- */
int gmsm_poly_eval(int group, const uint64_t *polys, const void *d_polys, const size_t *lens, size_t k, const uint64_t *point,
                   void *hip_stream, uint64_t *out_values);
int gmsm_poly_div_x_minus_a(int group, const uint64_t *poly, const void *d_poly, size_t n, const uint64_t *point,
                            void *hip_stream, uint64_t *out_h, void *d_out_h, uint64_t *out_value);
int gmsm_kzg_open(uint64_t handle, const uint64_t *poly, const void *d_poly, size_t n, const uint64_t *point,
                  void *hip_stream, uint64_t *out_claimed, uint64_t *out_h_jac);
int gmsm_kzg_open_folded(uint64_t handle, const uint64_t *polys, const void *d_polys, const size_t *lens, size_t k,
                         const uint64_t *point, const uint64_t *gamma, void *hip_stream, uint64_t *out_h_jac);

/* ---- shplonk.BatchOpen (ecc/<curve>/shplonk/shplonk.go:44-172) over registered G1 bases: polynomial i is opened on its own
 *      set S_i of npoints[i] points. Two stateless entries, one per Fiat-Shamir challenge (deriveChallenge stays with the
 *      caller, who bounces between them); results are bit-identical to the reference's. Polynomials as for the KZG
 *      entries: k fr.Element vectors concatenated (lens[i] coefficients each), exactly one of a host pointer / a 16-byte
 *      aligned device pointer produced on hip_stream, never modified. `points` holds sum_i npoints[i] fr.Element on the host,
 *      polynomial i's set first to last in the order given; out_claimed / claimed use the same layout. Every call
 *      returns when its results are complete; scratch comes from the workspace of the call.
 *   gmsm_shplonk_open_w (given gamma): out_claimed = f_i(s) for s in S_i; w = (sum_i gamma^i Z_(T\S_i) (f_i - r_i)) / Z_T,
 *      computed as sum_i gamma^i (f_i div Z_(S_i)) by a chain of npoints[i] divisions by (X - s) per polynomial, to exactly
 *      one of out_w (host) / d_out_w (device): maxlen = max_i lens[i] elements, zero above the true degree;
 *      out_w_jac = Commit(w) as Jacobian {X,Y,Z}.
 *   gmsm_shplonk_open_wprime (given z): out_wprime_jac = Commit(L / (X - z)), L = sum_i gamma^i Z_(T\S_i)(z) (f_i - r_i(z))
 *      - Z_T(z) w, with r_i interpolated from `claimed` and w (maxlen elements) from exactly one of w (host) / d_w (device,
 *      e.g. what gmsm_shplonk_open_w wrote).
 *   Both commitments go through the resident MultiExp (window tables included when the handle has them), over the true
 *   lengths only; the zero polynomial commits to infinity.
 *   Errors, all GMSM_ERR_ARG with a text: k == 0 or a null required pointer; both or none of a pair of pointers; an unknown
 *   handle or a handle of G2 bases; an empty polynomial; npoints[i] == 0; two equal points inside one S_i - a departure:
 *   the reference's interpolate inverts zero there and returns a meaningless proof without an error (equal points in
 *   different sets are legal); and the reference's size condition, checked up front in both entries: it commits wPrime
 *   over maxSizePolys + sum_i npoints[i] - 1 coefficients, maxSizePolys = max(max_i lens[i], max_i npoints[i] + 1)
 *   (shplonk.go:66-83, :163-166) - more than the registered size is "invalid polynomial size (larger than SRS or == 0)". ---- */
int gmsm_shplonk_open_w(uint64_t handle, const uint64_t *polys, const void *d_polys, const size_t *lens, size_t k,
                        const uint64_t *points, const size_t *npoints, const uint64_t *gamma, void *hip_stream,
                        uint64_t *out_claimed, uint64_t *out_w, void *d_out_w, uint64_t *out_w_jac);
int gmsm_shplonk_open_wprime(uint64_t handle, const uint64_t *polys, const void *d_polys, const size_t *lens, size_t k,
                             const uint64_t *points, const size_t *npoints, const uint64_t *claimed, const uint64_t *gamma,
                             const uint64_t *w, const void *d_w, const uint64_t *z, void *hip_stream, uint64_t *out_wprime_jac);

/* ---- fflonk (ecc/<curve>/fflonk/fflonk.go:41-141) over registered G1 bases: Fold, FoldAndCommit and the two halves of
 *      BatchOpen, which opens packs of polynomials. A pack of c polynomials is interleaved into one,
 *      Fold = sum_(j<t) P_j(X^t) X^j with t = getNextDivisorRMinusOne(c) (fflonk.go:234-252: the smallest divisor of r - 1
 *      that is >= c, at most 100 trials; P_j = 0 for c <= j < t), and opened by shplonk on the orbit {z, wz, .., w^(t-1) z}
 *      of each of its base points, w = g^((r-1)/t) with g the generator gmsm_fft_domain_info reports. Results are
 *      bit-identical to the reference's. Packs: all polynomials of all k packs concatenated (fr.Element vectors), lens[] one
 *      entry per polynomial, pack_sizes[k] each pack's polynomial count; exactly one of a host pointer / a 16-byte aligned
 *      device pointer produced on hip_stream, never modified. An empty member (lens == 0) of a non-empty pack is the zero
 *      polynomial. `points` holds sum_i npoints[i] BASE points on the host, pack after pack. Every call returns when its
 *      results are complete; scratch comes from the workspace of the call.
 *   gmsm_fflonk_next_divisor: t for n polynomials over the group's scalar field; host only.
 *   gmsm_fflonk_fold: Fold of one pack, t * max_j lens[j] elements to exactly one of out (host) / d_out (device).
 *   gmsm_fflonk_fold_commit: out_jac = Commit(Fold(pack)) as Jacobian {X,Y,Z} through the resident MultiExp over the folded
 *      length (an all-zero fold commits to infinity); the folded polynomial also goes to d_out_folded when that is not NULL.
 *   gmsm_fflonk_open_w (given gamma): with n_i = max length in pack i, a_k = z_k^t_i:
 *      out_claimed = ClaimedValues[i][j][k] = P_j(a_k): pack after pack t_i rows of npoints[i] values, rows j >= pack_sizes[i] zero;
 *      out_folded_claimed = SOpeningProof.ClaimedValues[i][k t_i + l] = Fold_i(w^l z_k): sum_i t_i npoints[i] elements;
 *      w = shplonk's w over the folded polynomials and the extended sets, computed as sum_i gamma^i Fold_i(P_j div
 *      prod_k (Y - a_k)) - t_i chains of npoints[i] divisions over n_i coefficients instead of one chain of t_i npoints[i]
 *      divisions over t_i n_i - to exactly one of out_w (host) / d_out_w (device): max_i t_i n_i elements, zero above the
 *      true degree; out_w_jac = Commit(w).
 *   gmsm_fflonk_open_wprime (given z): out_wprime_jac = Commit(L / (X - z)), L as for gmsm_shplonk_open_wprime over the
 *      folded polynomials (read from the packs in place, no folded copy), the extended sets, folded_claimed (the layout
 *      of out_folded_claimed) and w (max_i t_i n_i elements) from exactly one of w (host) / d_w (device).
 *   Errors, all GMSM_ERR_ARG with a text, all before any device work: k == 0 or a null required pointer; both or none of a
 *   pair of pointers; an unknown handle or a handle of G2 bases; pack_sizes[i] == 0; no divisor within 100 trials;
 *   npoints[i] == 0; a pack whose members are all empty (the folded polynomial is empty); two equal points in an extended
 *   set - z_a^t = z_b^t for a != b, or z = 0 with t_i > 1 (z = 0 with t_i = 1 is legal) - where the reference inverts zero;
 *   and shplonk's size condition over the FOLDED sizes, checked up front in both open entries: lengths t_i n_i and set sizes
 *   t_i npoints[i] in the condition of gmsm_shplonk_open_w - "invalid polynomial size (larger than SRS or == 0)", which
 *   gmsm_fflonk_fold_commit also returns for a fold longer than the registered size. ---- */
int gmsm_fflonk_next_divisor(int group, size_t n, size_t *out_t);
int gmsm_fflonk_fold(int group, const uint64_t *polys, const void *d_polys, const size_t *lens, size_t npolys, void *hip_stream,
                     uint64_t *out, void *d_out);
int gmsm_fflonk_fold_commit(uint64_t handle, const uint64_t *polys, const void *d_polys, const size_t *lens, size_t npolys,
                            void *hip_stream, void *d_out_folded, uint64_t *out_jac);
int gmsm_fflonk_open_w(uint64_t handle, const uint64_t *polys, const void *d_polys, const size_t *lens, const size_t *pack_sizes,
                       size_t k, const uint64_t *points, const size_t *npoints, const uint64_t *gamma, void *hip_stream,
                       uint64_t *out_claimed, uint64_t *out_folded_claimed, uint64_t *out_w, void *d_out_w, uint64_t *out_w_jac);
int gmsm_fflonk_open_wprime(uint64_t handle, const uint64_t *polys, const void *d_polys, const size_t *lens, const size_t *pack_sizes,
                            size_t k, const uint64_t *points, const size_t *npoints, const uint64_t *folded_claimed,
                            const uint64_t *gamma, const uint64_t *w, const void *d_w, const uint64_t *z, void *hip_stream,
                            uint64_t *out_wprime_jac);

/* ---- ToLagrangeG1 (ecc/<curve>/kzg/utils.go:25-64): the Lagrange form of an SRS, out[i] = (1/n) sum_j w^(-ij) P_j with
 *      w = fr.Generator(n) - for P_j = [tau^j]G that is [L_i(tau)]G - as an inverse FFT over G1 points on the device
 *      (gmsm_group_fft.h). Results are canonical affine limbs (infinity = (0, 0)), bit-identical to the reference's.
 *      G1 groups only: a G2 id is GMSM_ERR_ARG "ToLagrangeG1 is defined for G1 only".
 *   Precondition (as the reference's ScalarMultiplication, mulGLV): every input point lies in the r-torsion; the twiddle
 *      products use the GLV endomorphism (see GMSM_OPT_GLV).
 *   gmsm_to_lagrange_g1: n points in from exactly one of coeffs (host) / d_coeffs (device, 16-byte aligned, produced on
 *      hip_stream), out to exactly one of out_affine / d_out_affine; the output may alias the input. n = 1 returns the
 *      point unchanged (canonical). n == 0 or not a power of two: GMSM_ERR_ARG "len(coeffs) must be a power of 2"; n beyond
 *      the scalar field's 2-adicity: GMSM_ERR_ARG "m is too big: the required root of unity does not exist".
 *   gmsm_bases_to_lagrange: the Lagrange form of the first n bases of a registered handle (gmsm_bases_register*), computed
 *      from the resident points without a host round trip and registered as a NEW handle (an ordinary one:
 *      gmsm_bases_precompute, gmsm_multiexp_bases*, gmsm_bases_release). n larger than the handle's size, or an unknown
 *      handle: GMSM_ERR_ARG. Both calls return when the result is complete; scratch comes from the call's workspace. ---- */
int gmsm_to_lagrange_g1(int group, const uint64_t *coeffs, const void *d_coeffs, size_t n, void *hip_stream,
                        uint64_t *out_affine, void *d_out_affine);
int gmsm_bases_to_lagrange(uint64_t handle, size_t n, uint64_t *out_handle);

/* ---- mpcsetup updates (ecc/<curve>/mpcsetup, ecc/<curve>/kzg/mpcsetup.go): variable-base batch scalar multiplication on
 *      the device, one lane per point (gmsm_scale.h), for all six groups. Results are canonical affine limbs (infinity =
 *      (0, 0)), bit-identical to the reference's ScalarMultiplication followed by FromJacobian.
 *   Precondition (as the reference's ScalarMultiplication, mulGLV): every input point lies in the r-torsion; the walk uses
 *      the GLV endomorphism. Verify subgroup-checks first (gmsm_points_validate).
 *   Conventions of the three entries: n points in from exactly one of points (host) / d_points (device, 16-byte aligned,
 *      produced on hip_stream); inputs are not modified unless the output aliases them; the call returns when the result
 *      is complete; scratch comes from the call's workspace. An unknown group id is GMSM_ERR_ARG.
 *   gmsm_batch_scale: out[i] = scalars[i] * points[i] (n_scalars == n; Montgomery fr.Elements, from exactly one of scalars
 *      / d_scalars) or scalars[0] * points[i] (n_scalars == 1: the slice cases of mpcsetup.UpdateValues). Any other
 *      n_scalars: GMSM_ERR_LEN. Out to exactly one of out_affine / d_out_affine; the output may alias the input points.
 *      n == 0 is GMSM_OK and touches nothing. An input at infinity stays; scalar 0 gives infinity.
 *   gmsm_update_monomials: UpdateMonomialsG1, out[0] = points[0], out[i] = r^i * points[i], r one Montgomery fr.Element on
 *      the host; r^i is made on the device, no scalar vector exists. n < 2: GMSM_ERR_ARG (the reference indexes A[1]). The
 *      group id decides the point type: all six work (the reference's UpdateMonomialsG2 takes []G1Affine as generated).
 *   gmsm_linear_combinations: linearCombinationsG1/G2 (mpcsetup.go:396-447, :489-540). With `ends` the running ends of the
 *      segments of `points` (host, strictly increasing, ends[n_ends - 1] == n) and powers[i] = r^i over the flat index,
 *        truncated = sum r^i points[i]      over every i that is not the last of its segment,
 *        shifted   = sum r^i points[i + 1]  over the same i,
 *      as two MultiExps over device-made powers with zeros at ends[j] - 1; Jacobian {X,Y,Z} to host memory. The reference
 *      reaches `shifted` by way of r^-1 * truncated, the same group element for points in the r-torsion (the precondition
 *      above). GMSM_ERR_ARG before any device work: ends not strictly increasing, a segment shorter than 2 ("each slice
 *      must be of length at least 2"), ends[n_ends - 1] != n ("lengths mismatch"), a null required pointer. (linearCombinationG1
 *      /G2 with caller-supplied scalars is gmsm_multiexp.) ---- */
int gmsm_batch_scale(int group, const uint64_t *points, const void *d_points, size_t n,
                     const uint64_t *scalars, const void *d_scalars, size_t n_scalars,
                     void *hip_stream, uint64_t *out_affine, void *d_out_affine);
int gmsm_update_monomials(int group, const uint64_t *points, const void *d_points, size_t n, const uint64_t *r,
                          void *hip_stream, uint64_t *out_affine, void *d_out_affine);
int gmsm_linear_combinations(int group, const uint64_t *points, const void *d_points, size_t n,
                             const size_t *ends, size_t n_ends, const uint64_t *r, void *hip_stream,
                             uint64_t *out_truncated_jac, uint64_t *out_shifted_jac);

/* ---- fr.BatchInvert (ecc/<curve>/fr/element.go:658-687) and PLONK's accumulating-ratio polynomials
 *      (ecc/<curve>/fr/iop/ratios.go: BuildRatioCopyConstraint :136-246, BuildRatioShuffledVectors :45-127) on the device
 *      (gmsm_ratio.h): a factor kernel, two prefix-product scans run side by side, Montgomery's trick per tile, the expected
 *      form through the FFT and bit-reverse kernels. Results are bit-identical to the reference's: every output is a uniquely
 *      determined canonical fr.Element.
 *   Conventions, those of the KZG entries: Montgomery fr.Element limbs; exactly one of each host / device pointer pair;
 *      device pointers 16-byte aligned and produced on hip_stream; inputs are never modified; the call returns when its
 *      result is complete; scratch comes from the call's workspace. A G2 group id names its curve's scalar field as well.
 *   gmsm_fr_batch_invert: out[i] = 1 / a[i], and 0 where a[i] = 0 (the reference's zero rule). The output may alias the
 *      input. n == 0 is GMSM_OK and touches nothing.
 *   gmsm_iop_ratio_copy_constraint: `domain` is a gmsm_fft_domain_new handle and n its cardinality. `entries` holds m
 *      polynomials of n elements, concatenated, in LAGRANGE basis - the reference's ToLagrange on the inputs
 *      (polynomial.go:287-318) stays with the caller, through gmsm_fft - with layouts[j] (host) = 8 (Regular) or 16
 *      (BitReverse), the reference's values; `perm` holds m n int64 values in [0, m n). The result Z has Z_0 = 1 and
 *        Z_(i+1) = Z_i prod_j (P_j(w^i) + beta S[i + j n] + gamma) / (P_j(w^i) + beta S[perm[i + j n]] + gamma),
 *      S[p] = g^(p div n) w^(p mod n) the support of getSupportIdentityPermutation (g = FrMultiplicativeGen; read from the
 *      domain's twiddles, never built); where a denominator product is zero, Z is 0 from the next index on - what the
 *      reference's BatchInvert gives. Z is then put in the expected form (basis 1 Canonical, 2 Lagrange, 4 LagrangeCoset;
 *      layout 8 Regular, 16 BitReverse) as putInExpectedFormFromLagrangeRegular does (ratios.go:248-273) and written, n
 *      elements, to out / d_out. n = 1 returns [1] in the expected form.
 *   gmsm_iop_ratio_shuffled: Z_(i+1) = Z_i prod_j (beta - P_j(w^i)) / (beta - Q_j(w^i)) over m numerators and m
 *      denominators, each with its own layout; everything else as above.
 *   Errors are GMSM_ERR_ARG with a text, before any device work where the host can decide: m == 0; a null required
 *      pointer, or both or none of a pair; an unknown domain handle ("unknown fft domain handle"); an unknown basis or
 *      layout value; an output whose n elements overlap an input of a ratio entry, wholly or in part (host with host,
 *      device with device); a perm value outside [0, m n) - the reference panics
 *      there: "...: permutation[i] = v is outside [0, m n)" names the first such index (a permutation on the device is
 *      checked by the factor kernel; nothing is written to the output then).
 *   With gmsm_set_profiling(1) a ratio call adds its stage times to the slots 0 (factor kernel), 2 (the prefix products),
 *      5 (inversion and final multiply) and 6 (the transforms of the expected form) of gmsm_get_stage_times. ---- */
int gmsm_fr_batch_invert(int group, const uint64_t *a, const void *d_a, size_t n, void *hip_stream,
                         uint64_t *out, void *d_out);
int gmsm_iop_ratio_copy_constraint(uint64_t domain, const uint64_t *entries, const void *d_entries, size_t m,
                                   const uint32_t *layouts, const int64_t *perm, const void *d_perm,
                                   const uint64_t *beta, const uint64_t *gamma, int basis, int layout,
                                   void *hip_stream, uint64_t *out, void *d_out);
int gmsm_iop_ratio_shuffled(uint64_t domain, const uint64_t *num, const void *d_num, const uint64_t *den,
                            const void *d_den, size_t m, const uint32_t *num_layouts, const uint32_t *den_layouts,
                            const uint64_t *beta, int basis, int layout, void *hip_stream, uint64_t *out, void *d_out);

/* ---- iop.Polynomial (ecc/<curve>/fr/iop/polynomial.go) and iop.DivideByXMinusOne (quotient.go:21-79) on the device
 *      (gmsm_iop_poly.h): the rest of package iop, so that a polynomial the ratio entries read from HBM goes on to the
 *      coset of the big domain, through the quotient and to its evaluations without coming back to the host. Conventions,
 *      basis values (1 / 2 / 4) and layout values (8 / 16) are those of the ratio entries above; results are the reference's
 *      bit for bit.
 *   gmsm_iop_to_basis: (*Polynomial).ToLagrange / ToCanonical / ToLagrangeCoset (polynomial.go:287-390), IN PLACE (the one
 *      entry that modifies its argument). The buffer holds cardinality elements of which the first len are given; the call
 *      zeroes [len, cardinality) first - the reference's grow, which appends physically whatever the layout - also when the
 *      basis is already to_basis, then runs the transforms of the reference's switch (none, one, or two enqueued back to
 *      back with no host wait in between) and stores the layout the reference leaves in *out_layout: unchanged where
 *      nothing or two transforms run, flipped where one does. len == 0 gives cardinality zeros; len > cardinality is an
 *      error (the reference would hand fft a vector longer than the domain).
 *   gmsm_iop_evaluate: (*Polynomial).Evaluate (polynomial.go:104-132, 198-261) for k >= 1 polynomials of len coefficients
 *      each, concatenated, which share basis, size, shift and coset; layouts[j] (host) per polynomial; out_values (host)
 *      receives k elements. In the reference's order: basis LagrangeCoset: x <- x / coset with 0^-1 = 0 - a polynomial that
 *      never went through ToLagrangeCoset has coset 0 and is evaluated at 0, here as in the reference (coset may be NULL for
 *      the other bases); shift != 0: x <- x g^shift with g = fft.Generator(size), the generator of the next power of two
 *      >= size, not of len; Canonical basis: Horner over index i (Regular) or bitrev(i) (BitReverse); Lagrange and
 *      LagrangeCoset: barycentric, with w = fft.Generator(len),
 *        value = ((x^len - 1) / len) sum_i w^i c[idx(i)] / (x - w^i), 1/0 = 0 in the batch inversion.
 *      For x in the domain {w^i} the prefactor is zero and the result is 0: the reference's answer, NOT the interpolated
 *      value c[idx(i)]. Departure from the reference: a shift outside 0..5 is refused (GMSM_ERR_ARG); the reference
 *      multiplies x by an element it never initialised there and so evaluates at 0 - that defect is not reproduced.
 *   gmsm_iop_divide_by_x_minus_one: `a` holds N = card(domain_big) elements of a polynomial of size n = card(domain_small)
 *      in basis 4 (LagrangeCoset; any other basis: "the basis must be LagrangeCoset"), rho = N / n. For i in [0, N):
 *        out[bitrev(i)] = a.GetCoeff(i) inv[i mod rho], GetCoeff(i) = element (i + rho shift) mod N of a read through its
 *        layout (polynomial.go:151-163), inv[j] = 1 / (g^n t^j - 1), g = the big domain's FrMultiplicativeGen, t = its
 *        Generator^n (kept on the big domain per n after the first call),
 *      then FFTInverse(DIT, OnCoset) over the big domain: N elements in Canonical basis, Regular layout, to out / d_out.
 *   Errors are GMSM_ERR_ARG with a text, before any device work where the host can decide: both or none of a pair; an
 *      unknown basis or layout value (evaluate names the index: "layouts[j] = v is no layout"); an unknown domain handle
 *      ("unknown fft domain handle"); to_basis: len > cardinality, out_layout null; evaluate: k == 0, len == 0, size == 0,
 *      x / out_values null, coset null with basis 4, shift > 5, len no power of two in a Lagrange basis or with a
 *      BitReverse layout, len (Lagrange bases) or size (shift != 0) beyond the field's 2-adicity; quotient: domains of
 *      different curves, n > N, an output that overlaps the input wholly or in part. ---- */
int gmsm_iop_to_basis(uint64_t domain, uint64_t *a, void *d_a, size_t len, int basis, int layout, int to_basis,
                      void *hip_stream, int *out_layout);
int gmsm_iop_evaluate(int group, const uint64_t *polys, const void *d_polys, size_t k, size_t len, size_t size,
                      int basis, const uint32_t *layouts, unsigned shift, const uint64_t *coset, const uint64_t *x,
                      void *hip_stream, uint64_t *out_values);
int gmsm_iop_divide_by_x_minus_one(uint64_t domain_small, uint64_t domain_big, const uint64_t *a, const void *d_a,
                                   int basis, int layout, uint64_t shift, void *hip_stream, uint64_t *out, void *d_out);

/* ---- iop.Evaluate (ecc/<curve>/fr/iop/expressions.go:26-73) on the device (gmsm_iop_expr.h): a multivariate expression
 *      applied index by index to m polynomials of len elements each - the constraint numerator on the big coset, between
 *      gmsm_iop_to_basis and gmsm_iop_divide_by_x_minus_one, without a trip to the host. A Go closure cannot run on a GPU;
 *      an expression of this kind is a fixed sequence of field additions, subtractions and products, the same for every
 *      index, so the device form is a small straight-line PROGRAM, validated on the host and interpreted by one kernel, one
 *      index per lane.
 *   The program: prog_len words of uint32_t, one instruction per word: op | dst << 8 | a << 16 | b << 24. A lane owns the
 *      registers 0 .. GMSM_EXPR_MAX_REGS - 1, each one canonical Montgomery fr.Element. At index i:
 *        GMSM_EXPR_INPUT   dst <- x[a].GetCoeff(i)          GMSM_EXPR_CONST   dst <- consts[a] (n_consts elements, host)
 *        GMSM_EXPR_POINT   dst <- w^i, w = fft.Generator(len): the closure's argument i, which gnark's numerators use only
 *                          to index the domain's twiddles (any other function of i: pass it as one more input polynomial)
 *        GMSM_EXPR_ADD / _SUB / _MUL   dst <- reg[a] (+, -, x) reg[b]          GMSM_EXPR_NEG   dst <- -reg[a]
 *      The value of the expression is the dst of the last instruction. At most GMSM_EXPR_MAX_INSNS instructions,
 *      GMSM_EXPR_MAX_INPUTS inputs, GMSM_EXPR_MAX_CONSTS constants. Refused before any device work, each with a text that
 *      names the instruction index: an unknown opcode, a register >= 16, a read of a register that no earlier instruction
 *      wrote, an input index >= m or a constant index >= n_consts, POINT without a domain; and an empty or over-long program.
 *   polys / d_polys: a host array of m pointers (host / device), each to len elements; the inputs are NOT concatenated
 *      (resident wire polynomials are separate allocations). For i in [0, len), as GetCoeff does (polynomial.go:151-163):
 *        rho_j = len / sizes[j] (integer division), x_j(i) = element (i + rho_j shifts[j]) mod len of input j, read at that
 *        index for layouts[j] = 8 (Regular) and at its bit reversal for 16 (BitReverse);
 *        out[idx(i)] = f(i, x_0(i), ...), idx the identity for out_layout 8, the bit reversal for 16.
 *      The basis is a label only and stays with the caller. len may be any value >= 1 when every layout is Regular and the
 *      program has no POINT; else a power of two. With POINT, domain is a gmsm_fft_domain_new handle of the same curve whose
 *      cardinality is len (0: none). A G2 group id names its curve's scalar field.
 *   The output may be the same buffer as input j when layouts[j] == out_layout and that input's offset rho_j shifts[j] mod
 *      len is 0 - the lane that reads a slot is then the one that writes it; any other overlap of the output with an input,
 *      whole or partial, is refused (host with host, device with device). Inputs are never modified otherwise.
 *   len == 0 is GMSM_OK and touches nothing. Other errors are GMSM_ERR_ARG with a text: m == 0 ("need at least one input"),
 *      sizes[j] == 0 or > len, shifts[j] < 0 (the reference panics on the negative index), "layouts[j] = v is no layout", an
 *      unknown domain handle, a domain of another curve or cardinality, a null required pointer, both or none of a pair.
 *   With gmsm_set_profiling(1) the kernel's time goes to slot 0 of gmsm_get_stage_times. ---- */
#define GMSM_EXPR_INPUT 1
#define GMSM_EXPR_CONST 2
#define GMSM_EXPR_POINT 3
#define GMSM_EXPR_ADD 4
#define GMSM_EXPR_SUB 5
#define GMSM_EXPR_MUL 6
#define GMSM_EXPR_NEG 7
#define GMSM_EXPR_MAX_REGS 16
#define GMSM_EXPR_MAX_INSNS 4096
#define GMSM_EXPR_MAX_INPUTS 64
#define GMSM_EXPR_MAX_CONSTS 256
int gmsm_iop_evaluate_expression(int group, uint64_t domain, const uint32_t *prog, size_t prog_len, const uint64_t *consts,
                                 size_t n_consts, const uint64_t *const *polys, const void *const *d_polys, size_t m,
                                 size_t len, const size_t *sizes, const int64_t *shifts, const uint32_t *layouts,
                                 int out_layout, void *hip_stream, uint64_t *out, void *d_out);

/* ---- fr/polynomial.MultiLin (ecc/<curve>/fr/polynomial/multilin.go) and the sumcheck claim of one GKR wire
 *      (eqTimesGateEvalSumcheckClaims, ecc/<curve>/fr/gkr/gkr.go:143-348) on the device (gmsm_gkr.h): the prover side of
 *      the reference's second proving stack, whose loops run over the 2^n instances of a circuit. Conventions are those of
 *      the iop entries: Montgomery fr.Element limbs; a G2 group id names its curve's scalar field; exactly one of each host /
 *      device pointer pair; device pointers 16-byte aligned and produced on hip_stream; the call returns when its result is
 *      complete; every error the host can decide is GMSM_ERR_ARG with a text, before any device work, and nothing is
 *      written. Table lengths are powers of two, len = 2^n, and variable X_1 is the most significant bit of an index
 *      (multilin.go:14-17). Results are the reference's bit for bit: each is a uniquely determined canonical element.
 *   gmsm_multilin_fold: (*MultiLin).Fold, in place: a[i] <- a[i] + r (a[i + len/2] - a[i]) for i < len / 2; the elements
 *      [len/2, len) are not written (the reference leaves them as they were). len == 1 is refused: nothing to fold.
 *   gmsm_multilin_evaluate: (MultiLin).Evaluate: ncoords folds of a scratch copy, one after the other without a host wait,
 *      then element 0 to out_value (host). m is never modified. ncoords in [0, log2 len]; 0 returns m[0]. coords: host.
 *   gmsm_multilin_eq: (*MultiLin).Eq with m[0] = scale, and eqAcc (gkr.go:190-226) when accumulate != 0: for h < 2^n,
 *      v(h) = scale prod_{i<n} (bit_{n-1-i}(h) ? q[i] : 1 - q[i]); out[h] <- v(h), or out[h] <- out[h] + v(h). n == 0 gives
 *      out[0] = scale (or adds it). q, scale: host. Refused: n beyond what size_t indexes, a host output that overlaps q.
 *   A claim is a HANDLE that owns its tables in HBM between the rounds, because the Fiat-Shamir step between two rounds is the
 *      caller's. gmsm_shutdown releases every claim; gmsm_trim leaves them alone (their memory is in use).
 *   gmsm_gkr_claim_new: tables / d_tables is a host array of m pointers (host / device), each to len elements: the gate's
 *      input assignments (inputPreprocessors), in gate order; the same pointer may appear more than once. They are COPIED
 *      (gkr.go:397-403: folding destroys them); the caller's arrays are never modified. points (host): k >= 1 evaluation
 *      points of n = log2 len elements each; the claim's eq table is E = sum_{j<k} comb^j eq(points[j], .) (Combine,
 *      gkr.go:154-187); comb (host) is read only when k >= 2. prog is a GMSM_EXPR_* program (above) over the gate's inputs:
 *      INPUT a is gate input a < m, POINT is refused (a gate has no index), the value is the dst of the last instruction; it
 *      passes the same checks, with the same texts. degree is Gate.Degree(): an upper bound of the true degree, not checked
 *      against the program. out_gj (host) receives the first round polynomial, degree + 1 elements, on hip_stream, on
 *      which every later round of the claim runs too.
 *   The round polynomial (computeGJ): with the tables T_0 = E, T_1 .. T_m of current length L and half = L / 2,
 *      f_{t,d}(i) = T_t[i + half] + d (T_t[i + half] - T_t[i]) for d = 0 .. degree, and
 *      out_gj[d] = sum_{i<half} f_{0,d}(i) G(f_{1,d}(i), .., f_{m,d}(i)): g(1) .. g(degree + 1); g(0) is never sent.
 *   gmsm_gkr_claim_next: Next (gkr.go:296-317): every table is folded by r, then the round polynomial of the folded
 *      tables, in one pass. Refused when the tables have length 2: no variable is left, call gmsm_gkr_claim_final.
 *   gmsm_gkr_claim_final: the fold of ProveFinalEval (gkr.go:338): the m input tables, which must have length 2, are folded
 *      by r; out_evals (host) receives element 0 of each, m elements in input order (which of them become claims - the first
 *      occurrence of each distinct input wire - is the caller's business). Afterwards the handle accepts only release.
 *   Errors (GMSM_ERR_ARG, with a text): an unknown group; len zero or no power of two; len == 1 for a claim (the
 *      reference's sumcheck.Prove indexes an empty slice for zero variables); m == 0 or > GMSM_GKR_MAX_INPUTS; degree == 0 or
 *      > GMSM_GKR_MAX_DEGREE; k == 0; comb null with k >= 2; a null required pointer, both or none of a pair, a null table
 *      pointer ("tables[j] is null"); every program error; "unknown gkr claim handle"; "the claim is finished";
 *      next at length 2, final at another length; evaluate with ncoords > log2 len.
 *   The gate program's register file is in LDS and its operands are reloaded per point, so every valid program fits the
 *      kernel's budget: no claim is refused for its size. ---- */
#define GMSM_GKR_MAX_INPUTS 16
#define GMSM_GKR_MAX_DEGREE 15
int gmsm_multilin_fold(int group, uint64_t *a, void *d_a, size_t len, const uint64_t *r, void *hip_stream);
int gmsm_multilin_evaluate(int group, const uint64_t *m, const void *d_m, size_t len, const uint64_t *coords,
                           size_t ncoords, void *hip_stream, uint64_t *out_value);
int gmsm_multilin_eq(int group, const uint64_t *q, size_t n, const uint64_t *scale, int accumulate, void *hip_stream,
                     uint64_t *out, void *d_out);
int gmsm_gkr_claim_new(int group, const uint32_t *prog, size_t prog_len, const uint64_t *consts, size_t n_consts,
                       size_t degree, const uint64_t *const *tables, const void *const *d_tables, size_t m, size_t len,
                       const uint64_t *points, size_t k, const uint64_t *comb, void *hip_stream, uint64_t *out_gj,
                       uint64_t *out_handle);
int gmsm_gkr_claim_next(uint64_t handle, const uint64_t *r, uint64_t *out_gj);
int gmsm_gkr_claim_final(uint64_t handle, const uint64_t *r, uint64_t *out_evals);
int gmsm_gkr_claim_release(uint64_t handle);

/* ---- fr/mimc (ecc/<curve>/fr/mimc/mimc.go) and accumulator/merkletree over it (tree.go, verify.go) on the device
 *      (gmsm_mimc.h). Conventions are those of gmsm_fr_batch_invert: Montgomery fr.Element limbs; a G2 group id names its
 *      curve's scalar field; exactly one of each host / device pointer pair; device pointers 16-byte aligned and produced on
 *      hip_stream; the call returns when its result is complete; every error the host can decide is GMSM_ERR_ARG with a
 *      text, before any device work, and nothing is written. Digests are the reference's bit for bit.
 *   The hash (Miyaguchi-Preneel, mimc.go:130-163): h starts at the state (0 when none is given); for each element m:
 *      t <- m, then `rounds` times t <- (t + h + c_i)^5, then h <- (t + h) + h + m. rounds is 110 for BN254, 111 for
 *      BLS12-381, 163 for BW6-761; c_i: Keccak-256 chained from "seed", read big-endian mod r (initConstants).
 *   gmsm_mimc_constants: GetConstants. out (rounds elements, Montgomery limbs) and out_rounds may each be NULL, not both.
 *   gmsm_mimc_hash: the digest of len elements (host) continued from state (NULL: 0) to out (host), in host arithmetic: it
 *      never touches the device. This is the hash under a Fiat-Shamir transcript: a few blocks per challenge.
 *   gmsm_mimc_sum_batch: count digests: message i is the len elements at element offset i * stride, stride >= len; every
 *      message starts from state (host, NULL: 0). len == 0 gives count copies of the state. count == 0 is GMSM_OK and touches
 *      nothing. The output may not overlap the input.
 *   A tree is a HANDLE that owns every level of its sums in HBM (and its leaves' data with keep_leaves != 0). Leaf i is the
 *      leaf_len elements at i * leaf_len; its sum is their MiMC, a node is the MiMC of its two children (the reference's
 *      prefixes are commented out, tree.go:92-105), the shape is RFC 6962's for any n >= 1: an odd last node of a level moves up
 *      unchanged. gmsm_shutdown releases every tree; gmsm_trim leaves them alone (their memory is in use).
 *   gmsm_merkle_info: n, leaf_len and depth = ceil(log2 n), the longest path's number of siblings. NULL pointers are skipped.
 *   gmsm_merkle_root: the root's limbs to out_root (host).
 *   gmsm_merkle_prove: k paths in one gather launch. indices (host): k leaf indices. out_siblings (host): k * depth elements;
 *      path j's siblings bottom up from j * depth, out_counts[j] of them (a level where the node is the odd last one has no
 *      sibling), zeros behind. out_leaves (host, k * leaf_len elements; NULL: not wanted): the leaves' data, the first
 *      element of a reference proof set; allowed only if the leaves were kept. k == 0 is GMSM_OK.
 *   Errors (GMSM_ERR_ARG, with a text): an unknown group; a null required pointer, both or none of a pair; stride < len;
 *      sizes that do not fit; an output that overlaps the input; n == 0 or leaf_len == 0; out_leaves without kept leaves;
 *      an index >= n ("indices[j] = v is outside [0, n)"); "unknown merkle tree handle". ---- */
int gmsm_mimc_constants(int group, uint64_t *out, unsigned *out_rounds);
int gmsm_mimc_hash(int group, const uint64_t *state, const uint64_t *elems, size_t len, uint64_t *out);
int gmsm_mimc_sum_batch(int group, const uint64_t *msgs, const void *d_msgs, size_t count, size_t len, size_t stride,
                        const uint64_t *state, void *hip_stream, uint64_t *out, void *d_out);
int gmsm_merkle_new(int group, const uint64_t *leaves, const void *d_leaves, size_t n, size_t leaf_len, int keep_leaves,
                    void *hip_stream, uint64_t *out_handle);
int gmsm_merkle_info(uint64_t handle, size_t *out_n, size_t *out_leaf_len, unsigned *out_depth);
int gmsm_merkle_root(uint64_t handle, uint64_t *out_root);
int gmsm_merkle_prove(uint64_t handle, const uint64_t *indices, size_t k, uint64_t *out_leaves, uint64_t *out_siblings,
                      uint32_t *out_counts);
int gmsm_merkle_release(uint64_t handle);

/* ---- fr/fri's prover (ecc/<curve>/fr/fri/fri.go, RADIX_2_FRI with rho = 8) on the device (gmsm_fri.h). Conventions are those
 *      of the MiMC entries above. A FRI ORACLE is a handle that owns, in HBM, the sorted evaluations of every layer built so far
 *      (sorted[2i] = e[i], sorted[2i + 1] = e[i + s/2]: the reference's sort) and one MiMC Merkle tree per layer, leaf = one
 *      element. With N the domain's cardinality there are nb_steps = log2 N - 3 layers of N, N/2, ..., 16 elements. The
 *      Fiat-Shamir transcript stays with the caller: bind a root, derive x_i, fold. gmsm_shutdown releases every oracle;
 *      gmsm_trim leaves them alone. An oracle keeps its domain alive; one call at a time runs on an oracle.
 *   gmsm_fri_commit: domain is a gmsm_fft_domain_new handle with N >= 16. p (host) or d_p (device, produced on hip_stream): len <= N
 *      coefficients, zero padded to N, never modified. Runs FFT(DIF), BitReverse and sort as one transform and one gather, and
 *      builds the tree of layer 0.
 *   gmsm_fri_info: N, nb_steps and the number of folds done. NULL pointers are skipped.
 *   gmsm_fri_root: the root of layer `step`'s tree to out_root (host); step < the number of layers built.
 *   gmsm_fri_fold: foldPolynomialLagrangeBasis with the challenge xi (host) and the sort of its result in one pass: appends
 *      layer folds_done + 1 and its tree and writes the new root to out (host). The last fold (16 -> 8 elements) builds no tree:
 *      out receives the round's Evaluation.
 *   gmsm_fri_layer: the N >> step sorted evaluations of a layer to out (host) or d_out (device).
 *   gmsm_fri_query: the openings of a round in one launch and one copy back. positions (host): positions[i] is the queried
 *      leaf of layer i, i < count <= the number of layers built. All outputs are on the host. out_pairs: 2 * count elements,
 *      the leaves at positions[i] & ~1 and next to it. out_leaf_sums: count elements, the MiMC of leaf positions[i] (the
 *      neighbour's ProofSet[1]). out_siblings: count * log2 N elements, path i's siblings bottom up from i * log2 N,
 *      out_counts[i] of them, zeros behind. count == 0 is GMSM_OK.
 *   Errors (GMSM_ERR_ARG, with a text, nothing written): "unknown fft domain handle"; a cardinality below 16; len > N; both
 *      or none of p / d_p or of out / d_out; a null required pointer; a fold past nb_steps; a root, layer or query of a step
 *      that is not built; a position >= its layer's size; "unknown fri oracle handle". ---- */
int gmsm_fri_commit(uint64_t domain, const uint64_t *p, const void *d_p, size_t len, void *hip_stream, uint64_t *out_oracle);
int gmsm_fri_info(uint64_t oracle, uint64_t *out_cardinality, unsigned *out_nb_steps, unsigned *out_folds_done);
int gmsm_fri_root(uint64_t oracle, unsigned step, uint64_t *out_root);
int gmsm_fri_fold(uint64_t oracle, const uint64_t *xi, uint64_t *out);
int gmsm_fri_layer(uint64_t oracle, unsigned step, uint64_t *out, void *d_out);
int gmsm_fri_query(uint64_t oracle, const uint64_t *positions, size_t count, uint64_t *out_pairs, uint64_t *out_leaf_sums,
                   uint64_t *out_siblings, uint32_t *out_counts);
int gmsm_fri_release(uint64_t oracle);

/* ---- window-sharded pieces (multi-GPU: windows win_first, win_first+win_stride, ... of the c-bit decomposition are
 *      handled by this device; the tiny per-window totals are exchanged by the caller, e.g. one RCCL all-gather).
 *      out_xyzz (host) receives nwin_local x {X,Y,ZZ,ZZZ} extended-Jacobian window totals
 *      (= what processChunkG1Jacobian sends on chRes, multiexp_jacobian.go:60). ---- */
unsigned gmsm_default_window_bits(int group, size_t n);            /* the engine's choice of c for n points: a measured
                                                                      table per group, 8..17; c = 17 (BN254 G1 from 2^22
                                                                      points) is beyond the reference's uint16 digits */
unsigned gmsm_num_windows(int group, unsigned c);                  /* computeNbChunks, multiexp.go:681 */
/* What a MultiExp over n bases taken anew runs as under the current options: window width, number of windows,
 * entries_per_point (2 = GLV half scalars: 2 n entries per window, gmsm_glv.h; 1 = full scalars) and fused (1 = the fused
 * small-n kernel, 0 = the sorted pipeline). Cost only - the result does not depend on any of it. NULL pointers are skipped. */
int gmsm_default_plan(int group, size_t n, unsigned *c, unsigned *nwin, unsigned *entries_per_point, unsigned *fused);
/* c: 2..20 (the affine result does not depend on it, multiexp_test.go:95-126; the reference stops at 16); one call takes
 * up to 2^27 points for c <= 17 and 2^(44-c) beyond (32-bit sort entries) - larger inputs: split by point range and add
 * the sets with gmsm_fold_window_sets */
int gmsm_window_sums_device(int group, const void *d_points, const void *d_scalars, size_t n, unsigned c,
                            unsigned win_first, unsigned win_stride, void *hip_stream, uint64_t *out_xyzz);
/* The same pipeline without the copy-back: the nwin_local totals are written to the DEVICE buffer d_out_xyzz in stream
 * order and the call returns without waiting (the next step is an RCCL all-gather on the same stream; here hip_stream
 * NULL means the device's default stream, not an engine-private one). Bases: d_points
 * (Go layout) or, when bases_handle != 0, the registered bases (d_points ignored). */
int gmsm_window_sums_enqueue(int group, const void *d_points, uint64_t bases_handle, const void *d_scalars, size_t n,
                             unsigned c, unsigned win_first, unsigned win_stride, void *hip_stream, void *d_out_xyzz);
/* Point-sharded variant of the fold: xyzz_sets = nsets x nwin window totals, one set per point slice (every slice
 * decomposed with the same c). Window w = sum over the sets (g1JacExtended.add, g1.go:736), then the Horner fold. */
int gmsm_fold_window_sets(int group, unsigned c, const uint64_t *xyzz_sets, unsigned nsets, uint64_t *out_jac);
/* Horner fold of all nwin = gmsm_num_windows(group,c) window totals (msmReduceChunk, multiexp.go:302-315) -> Jacobian */
int gmsm_fold_windows(int group, unsigned c, const uint64_t *xyzz_windows, uint64_t *out_jac);
/* FromJacobian (g1.go:150-166) */
int gmsm_jac_to_affine(int group, const uint64_t *jac, uint64_t *out_affine);

/* ---- introspection / test hooks (used by tests/ to check each stage against the oracle) ---- */
size_t gmsm_affine_limbs(int group);   /* uint64 limbs of one affine point */
size_t gmsm_scalar_limbs(int group);
/* digits[nwin][n] (uint32 codes: 0 skip, d>0 -> 2d, d<0 -> 2(-d-1)+1) for host scalars; test hook for k_decompose */
int gmsm_debug_decompose(int group, const uint64_t *scalars, size_t n, unsigned c, uint32_t *out_digits);
/* test hook for the GLV split of gmsm_glv.h: out = n x 2 x (1 + half_words) uint32 - for scalar i (Montgomery fr limbs, as
 * everywhere) {sign of k1, |k1| words, sign of k2, |k2| words}, half_words = 4 (BN254), 5 (BLS12-381), 6 (BW6-761);
 * k1 + k2 lambda = s mod r (lambdaGLV, ecc/bn254/bn254.go:133) */
int gmsm_debug_glv_split(int group, const uint64_t *scalars, size_t n, uint32_t *out);
/* element-wise field ops on device: op 0 mul, 1 add, 2 sub, 3 neg, 4 dbl, 5 sqr, 6 from_mont; field 0 = fp, 1 = fr,
 * 2 = the group's coordinate field (Fp2 for G2 where applicable), 3 = the same coordinate field computed by the lazy-limb
 * code the pipeline uses (convert in, operate, convert out).  a,b,out: count x limbs host arrays. */
int gmsm_debug_field_op(int group, int field, int op, const uint64_t *a, const uint64_t *b, size_t count, uint64_t *out);
/* device group-law hook: out[i] = XYZZ accumulation of  acc[i] (+/-) pts[i]  (op 0 add_mixed, 1 sub_mixed),
 * op 2: out[i] = acc[i] + acc2[i] (xyzz add), op 3: out[i] = 2*acc[i]; ops 4..7: the same four through the lazy-limb
 * group law of the pipeline. */
int gmsm_debug_group_op(int group, int op, const uint64_t *acc, const uint64_t *pts_or_acc2, size_t count, uint64_t *out);

/* the launch shape of the bucket reduction over nw bucket sets of nbuckets buckets on the calling thread's device, under the
 * current options: out = {log2L, level-1 workgroups per set, workgroups of the second combine (0 = two levels), the combine
 * kernel of level 1 (1 k_combine_q, 2 k_combine_we), the serial kernel (0 one lane, 1 lane quads), the quads of k_reduce2_q} */
int gmsm_debug_reduce_shape(int group, uint32_t nw, uint32_t nbuckets, uint32_t out[6]);
/* the host fold over the plane sums of k_plane_sums (GMSM_OPT_REDUCE_TAIL = 2), no device needed: planes = nwin x
 * (7 + ceil(log2 nblocks1)) XYZZ values per window {Wsum, m_0..m_5, h_0..}; out_jac = sum_w 2^(c w) (Wsum_w +
 * sum_l 2^(log2L + l) m_l + sum_l 2^(log2L + 6 + l) h_l), infinity as (1, 1, 0) */
int gmsm_debug_fold_planes(int group, unsigned c, unsigned nwin, unsigned log2L, unsigned nblocks1, const uint64_t *planes,
                           uint64_t *out_jac);
/* what one run of the sorted pipeline derives on the host before it touches the device, no device needed: the layout of a
 * run over n points of the windows win_first, win_first + win_stride, ... of the c-bit decomposition (glv: of the half
 * scalars; shared: the one bucket set of window tables) on a device of num_cus compute units, under the current options.
 * flags = registered bases | totals stay on the device << 1 | stop after the fix-up << 2 | what the caller takes << 3 (0 window
 * totals, 1 plane sums when forced, 2 plane sums whenever they pay). out = GMSM_RUN_LAYOUT_WORDS integers, named in order by
 * "fields" of tests/golden/pipeline_layout.json; a run the pipeline would refuse is refused here with the same text. */
#define GMSM_RUN_LAYOUT_WORDS 51
int gmsm_debug_run_layout(int group, int num_cus, size_t n, unsigned c, unsigned win_first, unsigned win_stride, int glv, int shared,
                          unsigned flags, uint64_t *out);
unsigned long gmsm_debug_plane_runs(void); /* pipeline runs whose reduction ended in k_plane_sums so far (tests) */

/* ---- utilities ---- */
/* out_points[i] = [k0 + i*k1] * base, i < n (affine, Go layout). k0,k1: plain (non-Montgomery) little-endian limbs.
 * Host-side, nthreads worker threads. For building SRS-like synthetic bases (cf. BatchScalarMultiplicationG1,
 * ecc/bn254/g1.go:1039). */
int gmsm_generate_points(int group, const uint64_t *base_affine, const uint64_t *k0, const uint64_t *k1, int klimbs,
                         size_t n, int nthreads, uint64_t *out_points);
/* Per-stage device timing with HIP events on the launch streams. gmsm_set_profiling(1) resets and enables the
 * accumulators; gmsm_get_stage_times copies the summed milliseconds of up to max_stages stages
 * (0 base rewrite + decompose, 1 histogram, 2 scans, 3 scatter + fine sort, 4 bucket accumulation kernel, 5 split-bucket
 * fixup, 6 bucket reduction, 7 reserved = 0) and the number of pipeline runs they cover; returns the number of stages
 * written. gmsm_get_stage_launches gives how many stage instances each sum covers - for stage 4 that is the number of
 * k_accumulate_seg launches.  gmsm_set_profiling(2): only the accumulation kernel is bracketed (two events per pipeline
 * run instead of eight - the events themselves cost 0.03-0.05 ms per call): stage 4 and its launch count are filled,
 * the other stages stay 0. */
void gmsm_set_profiling(int on);
int gmsm_get_stage_times(double *out_ms, int max_stages, unsigned long *out_calls);
int gmsm_get_stage_launches(unsigned long *out_launches, int max_stages);

/* ---- switches (process-wide).  GMSM_OPT_WINDOW_BITS and GMSM_OPT_TABLES take their initial value from the environment
 *      variables GMSM_C / GMSM_TABLES once, when the library is first used; nothing reads the environment per call.
 *      GMSM_OPT_MAX_RUN / GMSM_OPT_HOST_RANGES exist for the tests of the point-range splits (0 = off),
 *      GMSM_OPT_POLY_LANE_BITS for the tests of the polynomial scan's launch shapes (0 = off),
 *      GMSM_OPT_REDUCE_SHAPE for the tests of the bucket reduction's launch shapes (0 = off). ---- */
enum gmsm_option {
    GMSM_OPT_WINDOW_BITS = 0, /* 0 = the library's measured table per group and size, 2..20 = forced (cost only: the
                                 affine result does not depend on c, multiexp_test.go:95-126) */
    GMSM_OPT_TABLES = 1,      /* window tables of registered bases: 0 never, 1 (default) the measured call sizes, 2 always */
    GMSM_OPT_MAX_RUN = 2,     /* lower the 2^27-point cap of one pipeline run: larger calls split into point ranges */
    GMSM_OPT_HOST_RANGES = 3, /* force the number of point ranges a host-buffer call is cut into */
    GMSM_OPT_FIXED_BASE_BITS = 4, /* table width of gmsm_batch_scalar_mul*: 0 = by batch size (8, and 11 from 2^21 scalars), 2..14 */
    GMSM_OPT_SPIN_WAIT_US = 5, /* a blocking MultiExp polls its stream for this many microseconds before it parks on it
                                 (default 0 = park at once; polling was measured at 5-6 us per call, 0.3-1 %, for a
                                 core kept busy as long as the call runs) */
    GMSM_OPT_SMALL_BITS = 6,  /* the fused small-n kernel (one launch, LDS buckets; calls of at most a few thousand points
                                 that neither force a window width nor are served by window tables): 0 (default) = on, width
                                 by size; 1 = off (the sorted pipeline for every size); 2..7 = on with this window width */
    GMSM_OPT_SMALL_MAX = 7,   /* largest call the fused small-n kernel takes (0 = the measured default) */
    GMSM_OPT_SPLIT = 8,       /* retired: still accepted and read back, no effect. It ran a call's windows as two groups on two streams;
                                 no gain (profiles/r05_split_groups.log), and the code is gone */
    GMSM_OPT_GLV = 9,         /* GLV half scalars (ecc/utils.go:62-170; s P = k1 P + k2 phi(P), half the windows and half the host
                                 fold for the same group element): 0 never; 1 (default) in the fused small-n kernel and, for
                                 bases taken anew, in the sorted pipeline at the sizes where it was measured ahead (2^13..2^20
                                 by group; nothing when a width is forced); 2 in every unregistered call (A/B).
                                 PRECONDITION while it is on - the one the reference's own mulGLV has (ecc/bn254/g1.go:536-600):
                                 phi(P) = [lambda]P holds on the r-torsion only. A point ON the curve but OUTSIDE the subgroup
                                 (possible where the cofactor is not 1: every group but BN254 G1; never a point that passed
                                 IsInSubGroup / the Decoder's default checks / gmsm_points_validate level 2) then contributes
                                 k1 P + k2 phi(P) instead of s P. The reference's MultiExp never uses the endomorphism and is
                                 the integer combination on ANY curve point: GMSM_OPT_GLV = 0 is exactly that
                                 (tests/test_gpu_glv.py::test_glv_off_is_the_integer_combination_outside_the_subgroup) */
    GMSM_OPT_SMALL_QUAD = 10, /* bucket phase of the fused small-n kernel on lane quads: 0 (default) by call size, 1 never,
                                 2 always (the Fp2 groups and BW6-761 always run it on quads) */
    GMSM_OPT_POLY_LANE_BITS = 11, /* for the tests of the suffix scan behind gmsm_poly_eval, gmsm_poly_div_x_minus_a, the gmsm_kzg_open
                                 and the gmsm_shplonk_open entries: 0 (default) = lanes of 8, 16 or 32 coefficients by length; k in 1..6 =
                                 lanes of 2^(k-1) coefficients whatever the length (a tile is 256 lanes, so k = 1 reaches the
                                 carry pass's lanes of several tiles at 2^16 coefficients instead of 2^21). Cost only: every
                                 output is the same field element. Read once per call. The prefix products and the batch inversion
                                 behind gmsm_fr_batch_invert and the gmsm_iop_ratio entries cut their vectors the same way. */
    GMSM_OPT_REDUCE_TAIL = 13, /* who applies the weights at the end of the bucket reduction. 1 = the device: the doubling ladders of
                                 k_combine_we / k_combine_q and k_reduce2_q leave one total per window, the host folds the windows.
                                 2 = the host: the device stops where its wide sums end (k_combine_we without its tail, then
                                 k_plane_sums: additions only, 7 + ceil(log2 blocks) sums per window written straight into the pinned
                                 result buffer) and the host fold adds every sum at its bit position in one Horner walk - where the
                                 shape allows it (a group that has k_combine_we, at most 128 first-level blocks, the result collected
                                 on the host: not gmsm_window_sums_enqueue, merged point ranges, window tables or the sharded
                                 exchange; the ladder elsewhere). 0 (default) = 2 for the MultiExp entries of the groups where it was
                                 measured ahead (BN254 G1) unless GMSM_OPT_REDUCE_SHAPE forces a shape, 1 elsewhere. Cost only: every
                                 result is the same group element. gmsm_debug_plane_runs counts the runs that took the host form. */
    GMSM_OPT_REDUCE_SHAPE = 12 /* for the tests of the bucket reduction's launch shapes: 0 (default) = the cost model. A packed value:
                                 bits 0-3 log2L (1..8 buckets per serial segment as a power of two, 0 = model), bits 4-5 the levels
                                 (2 = serial, combine, level 2; 3 = a second combine in between; 0 = model), bits 6-7 the combine kernel
                                 (1 = k_combine_q, 2 = k_combine_we where the group has it, 0 = by workgroup count). The planner still
                                 raises log2L until the last level holds its blocks, and runs two levels where three cannot be formed.
                                 Cost only: every window total is the same group element. gmsm_debug_reduce_shape reports the outcome. */
};
int gmsm_set_option(int key, unsigned value);
unsigned gmsm_get_option(int key);

/* ---- lifecycle.  Scratch buffers are grow-only per workspace (a steady stream of calls never allocates); the reference's
 *      per-call buffers are garbage-collected (ecc/bn254/multiexp.go:148-176), so a long-lived process needs the
 *      equivalent:  gmsm_trim releases every scratch / staging buffer larger than keep_bytes of every workspace that is
 *      idle right now, on every device (*out_freed = device bytes given back; registered bases, window tables and FFT
 *      domains stay).  gmsm_shutdown releases everything - handles become unknown, contexts, streams and events are
 *      destroyed - and leaves the library usable (state reappears on first use); no other call may run or start meanwhile,
 *      and it refuses (GMSM_ERR_ARG) while a submitted ticket is uncollected. ---- */
int gmsm_trim(size_t keep_bytes, size_t *out_freed);
int gmsm_shutdown(void);

int gmsm_device_count(void);
/* Device used by later calls of this thread AND process-wide default for threads that never called it (a goroutine
 * that is moved to another OS thread keeps its device as long as the process uses one device; a process that drives
 * several devices from several threads must pin them, runtime.LockOSThread). Entries that take device pointers or a
 * bases handle do not depend on it: they run on the device that owns the pointer / the registered bases.
 * Calling it also pins the drop-in entries to ONE device even when GMSM_DEVICES lists several
 * (gmsm_set_devices(NULL, 0) undoes that). */
int gmsm_set_device(int device);
/* text of the calling thread's last failure; a thread that never failed gets the most recent failure of the process
 * (a cgo caller may be rescheduled onto another OS thread between the failing call and this one) */
const char *gmsm_last_error(void);
const char *gmsm_version(void);

#ifdef __cplusplus
}
#endif
#endif /* GMSM_H */
