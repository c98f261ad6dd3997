// The sorted-bucket MultiExp pipeline of one (curve, group): what is computed on the host (RunLayout: a pure function of the
// CU count, the window plan, the point count, the request and the options - checkable without a device,
// gmsm_debug_run_layout), what is reserved (reserve) and what is launched, stage by stage (enqueue_window_sums). struct Group
// (gmsm_group.h) derives from it and decides which calls come here.
#pragma once
#include <algorithm>
#include <cstring>
#include <vector>

#include "gmsm_context.h"
#include "gmsm_group_host.h"
#include "gmsm_kernels.h"
#include "gmsm_fixup_q.h"
#include "gmsm_glv.h"

namespace gmsm {

// Tuning constants of the pipeline geometry. In the shipped library GMSM_TUNE(NAME, default) IS its default, folded at
// compile time - none of these is a run-time knob. An experiments build (-DGMSM_EXPERIMENTS, tools/build_ab.sh) reads
// GMSM_<NAME> from the environment instead, which is how the defaults below were swept:
//   LOG2L, REDUCE_LEVELS   buckets per serial reduction thread / two or three reduction levels (0 = the cost model)
//   SEG, SEGMAX            entries per accumulation thread (0 = chosen per launch) and its cap
//   PART_LOG2, STAGE_CAP   coarse partition population, staging slots of the fine sort
//   DEVICE_RANGES          point ranges of a device-resident call beyond the pipeline-run cap
#define GMSM_TUNE(NAME, DFLT) tune_uint("GMSM_" #NAME, (DFLT))

template <class T> struct LazyOf;
template <class P> struct LazyOf<Fp<P>> { using type = FpU<P>; };
template <class P> struct LazyOf<Fp2<P>> { using type = Fp2U<P>; };

// GMSM_OPT_REDUCE_TAIL: what a caller of enqueue_window_sums can take from ws.pinned - window totals only, plane sums
// when the option forces them (it converts them to totals itself: collect_window_sums), plane sums whenever they pay
// (it folds on the host: collect_folded).
enum { TAIL_LADDER = 0, TAIL_IF_FORCED = 1, TAIL_AUTO = 2 };

// What a caller asks of one pipeline run beyond its inputs.
struct RunRequest {
    void *d_out = nullptr;        // the totals stay on the device (copied here in stream order) instead of going to ws.pinned
    size_t resident_offset = 0;   // first registered base used
    bool buckets_only = false;    // stop after the fix-up: ws.buckets / ws.starts hold the range's bucket sums (a range of a
                                  // multi-range call: k_merge_buckets adds them to the running buckets, enqueue_reduce ends it)
    bool time_range = false;      // buckets_only: the caller collects the stage events of this range before it enqueues the next
    int tail_mode = TAIL_LADDER;  // what the caller can take from ws.pinned
};

template <class F_, class FrP_, class Consts_>
struct Pipeline : GroupHost<F_, FrP_> {
    using Host = GroupHost<F_, FrP_>;
    using Host::fold;
    using Host::fold_planes;
    using F = F_;
    using FrP = FrP_;
    using Consts = Consts_;  // curve coefficient, wire-format flag bits (gmsm_params32.h)
    using Aff = Affine<F>;
    using Ext = XYZZ<F>;
    using J = Jac<F>;
    static constexpr unsigned FR_BITS = FrP::BITS;
    static constexpr size_t AFF_BYTES = sizeof(Aff);
    // unsaturated-limb accumulation (gmsm_fieldu.h) for groups whose coordinates live in Fp; Fp2 groups use the generic
    // saturated kernel
    using U = typename LazyOf<F>::type;  // lazy element type: FpU<P> for Fp coordinates, Fp2U<P> for Fp2 coordinates
    // Group operations are inlined where a kernel has ONE call site of the addition (k_accumulate_seg, k_fixup_seg,
    // k_reduce_serial: a single inlined Fp2 or BW6-761 addition is 60-350 KB of code); everything that combines few
    // elements (long chains, the reduction's combine and level 2) runs on lane quads with the operands in LDS (gmsm_quad.h).
    using OpsSerial = UnsatOps<U>;
    static constexpr size_t REC = sizeof(typename OpsSerial::Mem);  // bucket / partial record (lazy representation on the fast path)
    // Level 1 of the bucket reduction = k_reduce_serial (one thread per L buckets, no LDS) + k_combine_q (COMBINE_N
    // (S, W) pairs per workgroup of 4 * COMBINE_N threads); level 2 = k_reduce2_q, at most RED2_TPB level-1 results per window.
#ifndef GMSM_FORK_CONVERT_LOG2
#define GMSM_FORK_CONVERT_LOG2 18
#endif
    static constexpr size_t FORK_CONVERT_MIN = (size_t)1 << GMSM_FORK_CONVERT_LOG2;  // unregistered calls from here on rewrite their bases on a side stream
    static constexpr int COMBINE_N = 64;
    static constexpr int RED2_TPB = 64;
    // The serial part itself runs on quads (k_reduce_serial_q) for every element type but the 9-limb prime field.
    // Measured reduce times one-lane / quad serial (same box): BW6-761 2^20 1.85 / 1.13 ms, BLS12-381 G2 2^22 2.17 / 1.61,
    // BN254 G2 2^20 0.955 / 0.906, BLS12-381 G1 2^22 0.675 / 0.601 (2^16: 0.688 / 0.611).
#ifndef GMSM_SERIAL_QUAD_WORDS
#define GMSM_SERIAL_QUAD_WORDS 14
#endif
    static constexpr bool SERIAL_QUAD = sizeof(U) >= GMSM_SERIAL_QUAD_WORDS * 4;
#ifndef GMSM_SERIAL_Q_QUADS
#define GMSM_SERIAL_Q_QUADS 64
#endif
    static constexpr int SERIAL_Q_QUADS = GMSM_SERIAL_Q_QUADS;  // quads per workgroup of k_reduce_serial_q (A/B: tools/build_ab.sh)
    // The work-efficient combine (k_combine_we: half the issue work, one step more) where the combine is throughput-bound:
    // the 9-limb field with at least two workgroups per CU. Measured k_combine_q / k_combine_we reduce times, BN254 G1:
    // 2^16 0.293 / 0.277 ms, 2^18 0.337 / 0.308, 2^20 0.344 / 0.312, 2^24 0.465 / 0.433 - but 2^12 (a handful of
    // workgroups: latency) 0.080 / 0.106, and the 14-limb field 0.628 / 0.68 (three workgroups per CU, not four).
#ifndef GMSM_COMBINE_WE_WORDS
#define GMSM_COMBINE_WE_WORDS 9
#endif
    static constexpr bool COMBINE_WE = sizeof(U) <= GMSM_COMBINE_WE_WORDS * 4;
    // GMSM_OPT_REDUCE_SHAPE (tests) names the combine kernel in bits 6-7: 1 = k_combine_q, 2 = k_combine_we where it is compiled
    static bool use_combine_we(int num_cus, uint32_t workgroups) {
        const unsigned forced = (options().reduce_shape.load(std::memory_order_relaxed) >> 6) & 3u;
        if (forced) return COMBINE_WE && forced == 2;
        return COMBINE_WE && workgroups >= 2u * (uint32_t)num_cus;
    }
    // k_fixup_seg: followers a chain head adds itself (one-lane additions); longer chains go to k_fixup_long (quads, one
    // workgroup per chain). Handing chains of 3+ links to the quads for the wide types was measured: no gain at 2^20
    // (BW6-761 fixup 0.75 ms either way - it is 322 K two-link chains in five rounds of 512-register workgroups), and 2^16
    // got slower (0.68 -> 2.6 ms: thousands of short chains, one workgroup each).
    static constexpr uint32_t FIX_MAXWALK = FIXUP_MAXWALK;
    // k_fixup_seg on lane quads (gmsm_fixup_q.h) for the element types whose one-lane addition spills: everything wider than
    // the 14-limb prime field (BN254 G2, BLS12-381 G2, BW6-761). -DGMSM_FIXUP_QUAD_WORDS=1000 builds the one-lane form (A/B).
#ifndef GMSM_FIXUP_QUAD_WORDS
#define GMSM_FIXUP_QUAD_WORDS 15
#endif
    static constexpr bool FIXUP_QUAD = sizeof(U) >= GMSM_FIXUP_QUAD_WORDS * 4;
    // plan_reduction: combine workgroups resident on a CU (measured on the pieces of a window-sharded call and on single
    // bucket sets, profiles/r03_reduce_levels.log: with one per CU the model kept few windows on the two-level form)
    static constexpr size_t COMBINE_RESIDENT = sizeof(U) <= 36 ? 4 : sizeof(U) <= 56 ? 3 : sizeof(U) <= 72 ? 2 : 1;
#ifndef GMSM_PLANES_AUTO_WORDS
#define GMSM_PLANES_AUTO_WORDS 9
#endif
    // groups whose MultiExp entries take the host planes by default: BN254 G1 (the 9-limb field), measured in
    // profiles/reduce_planes_ab.md; the plane kernels exist for the groups that have k_combine_we
    static constexpr bool PLANES_AUTO = sizeof(U) <= GMSM_PLANES_AUTO_WORDS * 4;
    // first-level blocks per window the plane form takes (tested up to here). BN254 G1 at 2^20 - GLV half scalars, c = 16,
    // 2^16 buckets, L = 8 - has 128; more would be a three-level plan at small L, which the cost model leaves to few windows.
    static constexpr uint32_t PLANE_BLOCKS = 128;

    // ------------------------------------------------------------------ window plans
    static WindowPlan make_plan(unsigned c, unsigned win_first, unsigned win_stride) {
        WindowPlan p;
        p.c = c;
        p.nwin_total = num_windows(FR_BITS, c);
        unsigned lc = last_c(FR_BITS, c);
        p.nbuckets = 1u << (std::max(c, lc) - 1);
        p.win_first = win_first;
        p.win_stride = win_stride ? win_stride : 1;
        p.nwin_local = win_first < p.nwin_total ? (p.nwin_total - win_first + p.win_stride - 1) / p.win_stride : 0;
        p.shared = 0;
        p.glv = 0;
        return p;
    }
    // the windows of the GLV half scalars (gmsm_glv.h): same rules over GLV_BITS bits
    static constexpr unsigned GLV_BITS = (unsigned)FrP::GLV_BITS;
    static WindowPlan make_plan_glv(unsigned c, unsigned win_first, unsigned win_stride) {
        WindowPlan p = make_plan(c, win_first, win_stride);
        p.nwin_total = num_windows(GLV_BITS, c);
        p.nbuckets = 1u << (std::max(c, last_c(GLV_BITS, c)) - 1);
        p.nwin_local = win_first < p.nwin_total ? (p.nwin_total - win_first + p.win_stride - 1) / p.win_stride : 0;
        p.glv = 1;
        return p;
    }
    // widths k_decompose_glv is instantiated for
    static bool glv_width_built(unsigned c) { return (c >= 10 && c <= 18) || c == 20; }
    // bucket sets of a run: what the sort, the accumulation and the reduction see as windows (window tables: ONE set)
    static uint32_t bucket_sets(const WindowPlan &plan) { return plan.shared ? 1u : plan.nwin_local; }

    // floor(r / 2^shift) for the scalar-field modulus r (the largest value a top window can hold, before the carry)
    static uint64_t fr_modulus_shifted(unsigned shift) {
        uint64_t v = 0;
        for (int b = 62; b >= 0; --b) {
            const unsigned bit = shift + (unsigned)b;
            if (bit < 32u * FrP::N && ((FrP::Q[bit >> 5] >> (bit & 31)) & 1u)) v |= (uint64_t)1 << b;
        }
        return v;
    }
    // largest digit code k_decompose can emit for this plan (multiexp.go:779-800): decides uint16 vs uint32 digit arrays
    static uint64_t max_digit_code(const WindowPlan &plan) {
        if (plan.glv) {  // half scalars below 2^GLV_BITS: the top window holds at most 2^(its bits) (value + carry), code = 2 digit
            const uint64_t low = ((uint64_t)1 << plan.c) - 1;
            const unsigned top_bits = GLV_BITS - (plan.nwin_total - 1) * plan.c;
            return std::max(low, (uint64_t)2 << top_bits);
        }
        const uint64_t low = ((uint64_t)1 << plan.c) - 1;
        const unsigned top_shift = (plan.nwin_total - 1) * plan.c;
        const uint64_t top = top_shift >= 63 + 32u * FrP::N ? 0 : ((fr_modulus_shifted(top_shift) + 1) << 1);
        return plan.nwin_total > 1 ? std::max(low, top) : top;
    }

    // ------------------------------------------------------------------ the plan of one run (host arithmetic only)
    // Accumulation and reduction geometry of one pipeline run over nw windows of n points.
    struct Geometry {
        uint32_t seg, tpw;                     // accumulation: entries per thread, threads per window
        uint32_t log2L, nblocks1, log2span;    // reduction: buckets per serial thread, level-1 workgroups per window
        uint32_t nblocks2;                     // 0: serial - combine - level 2; else a second combine of nblocks2 workgroups
        uint32_t T;                            // (S, W) pairs per window of k_reduce_serial
        uint32_t plane_h;                      // plane form: ceil(log2 nblocks1), the planes above the combine's seven
    };
    static Geometry plan_geometry(int num_cus, uint32_t nw, size_t n, uint32_t NB, bool shared_set = false) {
        Geometry q;
        plan_reduction(num_cus, nw, NB, q);
        plan_accumulation(num_cus, nw, n, NB, shared_set, q);
        return q;
    }
    // reduction: buckets per serial thread, L = 2^log2L; COMBINE_N of their (S, W) pairs per combine workgroup; the
    // last level (k_reduce2_q) takes at most RED2_TPB blocks per window, one quad each. Few windows of many buckets
    // (one rank's share of a window-sharded call, the single bucket set of the window tables) would need a long
    // serial walk to get there: a second combine level in between keeps L short.
    static void plan_reduction(int num_cus, uint32_t nw, uint32_t NB, Geometry &q) {
        constexpr size_t SPAN1 = COMBINE_N;  // pairs one combine workgroup takes
        const auto blocks1 = [&](uint32_t l2) { return ((size_t)NB + (SPAN1 << l2) - 1) / (SPAN1 << l2); };
        const auto blocks2 = [&](uint32_t l2) { return (blocks1(l2) + SPAN1 - 1) / SPAN1; };
        // GMSM_OPT_REDUCE_SHAPE (tests; 0 = off): log2L in bits 0-3, the number of levels in bits 4-5
        const unsigned forced_shape = options().reduce_shape.load(std::memory_order_relaxed);
        uint32_t log2L = GMSM_TUNE(LOG2L, forced_shape & 15u);
        const uint32_t force_levels = GMSM_TUNE(REDUCE_LEVELS, (forced_shape >> 4) & 3u);  // 2 / 3; 0 = cost model
        bool three = force_levels == 3;
        if (log2L == 0) {
            // serial kernel: 2L dependent one-lane additions on every SIMD, as many rounds as the threads need;
            // combine: 2 log2 N + log2 L + 1 quad steps (a quad step is about a third of a one-lane addition) per
            // round of workgroups. Minimise the total in units of one-lane additions.
            // The width of the TWO-level form is chosen with one combine workgroup per CU and round - the model all
            // full-call configurations were measured with. Whether a second combine level pays is then decided with
            // the workgroups a CU really holds at once (COMBINE_RESIDENT; their steps interleave): with one per CU the
            // model kept few windows on a long serial walk (2^20 piece of 8: reduce 0.221 ms, 0.176 with three levels;
            // 2^24 piece of 4: 0.358 / 0.271 - profiles/r03_reduce_levels.log).
            const auto costs = [&](uint32_t l2, size_t resident, size_t *c3) {
                const size_t serial_threads = (size_t)nw * (((size_t)NB + ((size_t)1 << l2) - 1) >> l2);
                // lanes of the serial kernel: one per thread, or a quad per thread at a third of the step time
                const size_t serial_lanes = SERIAL_QUAD ? 4 * serial_threads : serial_threads;
                const size_t serial_rounds = (serial_lanes + (size_t)num_cus * 256 - 1) / ((size_t)num_cus * 256);
                const size_t per_round = (size_t)num_cus * resident;
                const size_t rounds = ((size_t)nw * blocks1(l2) + per_round - 1) / per_round;
                const size_t cost_serial = (SERIAL_QUAD ? 1 : 3) * serial_rounds * ((size_t)2 << l2);
                const size_t c2 = cost_serial + rounds * (2 * 6 + l2 + 1);
                // second combine: its own rounds of 2 * 6 + 1 steps + the tail of the prescaling, and one more launch
                const size_t rounds_b = ((size_t)nw * blocks2(l2) + per_round - 1) / per_round;
                *c3 = c2 + rounds_b * (2 * 6 + 8) + 4;
                return c2;
            };
            size_t best2 = ~(size_t)0, best3 = ~(size_t)0, unused = 0;
            uint32_t l2_two = 0, l2_three = 0;
            for (uint32_t l2 = 1; l2 <= 8; ++l2) {
                const size_t c2 = costs(l2, 1, &unused);
                if (blocks1(l2) <= (size_t)RED2_TPB && c2 < best2) {
                    best2 = c2;
                    l2_two = l2;
                }
                size_t c3 = 0;
                (void)costs(l2, COMBINE_RESIDENT, &c3);
                if (blocks1(l2) > 1 && blocks2(l2) <= (size_t)RED2_TPB && c3 < best3) {
                    best3 = c3;
                    l2_three = l2;
                }
            }
            const size_t two_resident = l2_two ? costs(l2_two, COMBINE_RESIDENT, &unused) : ~(size_t)0;
            if (force_levels == 3 ? l2_three != 0 : (force_levels != 2 && l2_three != 0 && best3 < two_resident)) {
                log2L = l2_three;
                three = true;
            } else if (l2_two) {
                log2L = l2_two;
                three = false;
            } else {
                log2L = 8;
            }
        } else if (three && blocks1(log2L) <= 1) {
            three = false;  // a forced width with three levels asked for: one combine workgroup leaves nothing for a second level
        }
        if (three) {
            while (blocks2(log2L) > (size_t)RED2_TPB) ++log2L;
        } else {
            while (blocks1(log2L) > (size_t)RED2_TPB) ++log2L;
        }
        q.log2L = log2L;
        q.nblocks1 = (uint32_t)blocks1(log2L);
        q.nblocks2 = three ? (uint32_t)blocks2(log2L) : 0u;
        q.log2span = log2L;
        for (size_t t = SPAN1; t > 1; t >>= 1) ++q.log2span;
        q.T = (uint32_t)(((size_t)NB + ((size_t)1 << log2L) - 1) >> log2L);
        q.plane_h = 0;
        while ((1u << q.plane_h) < q.nblocks1) ++q.plane_h;
    }
    // entry-parallel segmented accumulation: seg entries per thread. Every thread does the same work, so the
    // launch should be a whole number of resident "rounds" of WORKGROUPS: the grid is (blocks per window) x
    // (windows), so the unit is a 256-thread block per window - nw * ceil(tpw/256) blocks must not exceed
    // rounds x (CUs x resident blocks). (Counting threads instead put 24 x 11 = 264 blocks on 256 CUs for the
    // 24 windows of BW6-761: eight blocks ran a second round alone and the kernel took twice as long - PMC:
    // 1056 waves, each alive for half of the kernel.) Among the round counts that keep seg <= SEG_MAX the
    // one that fills its last round best is taken.
    static void plan_accumulation(int num_cus, uint32_t nw, size_t n, uint32_t NB, bool shared_set, Geometry &q) {
        uint32_t seg = GMSM_TUNE(SEG, 0);
        if (seg == 0) {
            const size_t cap_blocks = (size_t)num_cus * AccWaves<U>::value;
            const size_t SEG_MAX = GMSM_TUNE(SEGMAX, 512);  // measured: 512 best at 2^24, 256 at 2^22
            // Shortest segment. A launch that does not fill the chip is a latency chain of `seg` additions per thread:
            // with sparse buckets (<= 8 entries each: few chains of partial sums to close) shorter segments on more
            // threads win - BN254 G1 2^14 0.605 -> 0.476 ms, 2^16 0.637 -> 0.585, BLS12-381 G1 2^16 1.17 -> 0.98; crowded
            // buckets (the 8-bit windows of small inputs) would pay it back in the fix-up (BLS12-381 G1 2^14: 0.13 -> 0.49 ms).
            // Measured for the three narrow element types (profiles/r03_short_segments.log).
            size_t seg_floor = 32;
            if (sizeof(U) <= 72 && n / NB <= 8) {
                const size_t entries = (size_t)nw * n, cap_threads = cap_blocks * 256;
                seg_floor = entries / 8 <= cap_threads ? 8 : entries / 16 <= cap_threads ? 16 : 32;
            } else if (sizeof(U) <= 72 && shared_set) {
                // the shared bucket set of the window tables is crowded by construction, but its chains are closed one
                // thread per bucket (k_fixup_bucket): BN254 G1 2^14 0.456 -> 0.365 ms at 8, 2^16 0.472 -> 0.400 at 16
                // (0.428 at 8), 2^17 and up best at 32; BLS12-381 G1 2^15 0.775 -> 0.601 at 8, 2^16 0.817 -> 0.657 at 16;
                // BN254 G2 (its one-lane additions cost three times as much) 2^15 1.088 -> 0.824 at 16, 2^16 best at 32
                const size_t entries = (size_t)nw * n;
                if (sizeof(U) <= 56) seg_floor = entries <= ((size_t)1 << 19) ? 8 : entries <= ((size_t)3 << 19) ? 16 : 32;
                else seg_floor = entries <= ((size_t)3 << 18) ? 16 : 32;
            }
            size_t best_seg = 0, first_r = 0;
            double best_fill = -1.0;
            for (size_t r = 1; r < 100000; ++r) {
                const size_t bpw = r * cap_blocks / nw;  // whole blocks per window in r rounds
                if (bpw == 0) continue;
                const size_t sg = std::max<size_t>((n + bpw * 256 - 1) / (bpw * 256), seg_floor);
                if (sg > SEG_MAX) continue;
                if (!first_r) first_r = r;
                const size_t blocks = (size_t)nw * (((n + sg - 1) / sg + 255) / 256);
                const double fill = (double)blocks / (double)(((blocks + cap_blocks - 1) / cap_blocks) * cap_blocks);
                if (fill > best_fill + 1e-9) {
                    best_fill = fill;
                    best_seg = sg;
                }
                if (fill > 0.985 || r >= first_r + 5 || sg == seg_floor) break;
            }
            seg = (uint32_t)(best_seg ? best_seg : seg_floor);
        }
        q.seg = seg;
        q.tpw = (uint32_t)((n + seg - 1) / seg);  // threads per window (upper bound: <= n entries)
    }
    // scratch of the reduction for nw bucket sets: the level-1 (and level-2) results - or, plane form, the combine's eight
    // sums per block -, and the serial kernel's pairs
    static size_t partials_bytes(const Geometry &q, uint32_t nw, bool planes) {
        const size_t tot_blk = (size_t)nw * q.nblocks1;
        return planes ? tot_blk * 8 * REC : (tot_blk + (size_t)nw * q.nblocks2) * 2 * REC;
    }
    static size_t red_pre_bytes(const Geometry &q, uint32_t nw) { return (size_t)nw * q.T * 2 * REC; }
    // quads of k_reduce2_q: a power of two, at least 2, that holds the nlast results of the last combine level
    static uint32_t reduce2_active(uint32_t nlast) {
        uint32_t active = 2;
        while (active < nlast) active <<= 1;
        return active;
    }
    // gmsm_debug_reduce_shape: what the reduction of nw bucket sets of NB buckets is launched as under the current options -
    // log2L, nblocks1, nblocks2, the (first) combine kernel (1 k_combine_q, 2 k_combine_we), the serial kernel (0 one lane,
    // 1 quads), the quads of k_reduce2_q. (The number of entries only shapes the accumulation.)
    static void reduce_shape(int num_cus, uint32_t nw, uint32_t NB, uint32_t out[6]) {
        Geometry q;
        plan_reduction(num_cus, nw, NB, q);
        out[0] = q.log2L;
        out[1] = q.nblocks1;
        out[2] = q.nblocks2;
        out[3] = use_combine_we(num_cus, q.nblocks1 * nw) ? 2u : 1u;
        out[4] = SERIAL_QUAD ? 1u : 0u;
        out[5] = reduce2_active(q.nblocks2 ? q.nblocks2 : q.nblocks1);
    }

    // Everything enqueue_window_sums derives from its arguments before it touches the device.
    struct RunLayout {
        const char *error;         // the refusal (GMSM_ERR_ARG) this run ends with, or nullptr
        uint32_t nw, nwd;          // bucket sets; windows of the digit decomposition = totals handed out
        size_t n, n_points;        // sort entries per bucket set; scalars / bases of this run
        bool shared, glv;          // window tables: ONE set of nwd * n_points entries; half scalars: two entries per point
        bool d16;                  // uint16 digit codes
        bool fork_convert;         // unregistered bases are rewritten on a side stream beside the scalar pipeline
        Geometry q;
        bool planes;               // GMSM_OPT_REDUCE_TAIL: the reduction stops at its plane sums, the host fold scales them
        uint32_t plane_np;         // planes per window of that form: 7 + q.plane_h
        // sort: 2^fbits fine buckets per coarse partition, nparts partitions, pchunks chunks of pchunk_len entries
        uint32_t log2NB, lidx, part_log2, fbits, nparts, pchunks, stage_cap, hcap, scap, heavy_wg;
        bool big_chunk;
        size_t pchunk_len, scatter_lds, list_cap;
        // bytes of every scratch buffer (ws.<name>), the pinned result buffer, and the offsets carved out of three of them
        size_t digits, sorted, parted, starts, buckets, partials, red_pre, totals, pinned, blockhist, counts, seg_partials, seg_flags,
            seg_bucket, seg_lvl, long_pieces, heavy, upoints;
        size_t piece_sums_off, hparts_bytes, hcount_bytes;
    };
    // The refusals keep this order: GLV over registered bases, 2^31 entries, the three of the sort geometry, 256 windows.
    static RunLayout plan_run(int num_cus, const WindowPlan &plan, size_t n, bool resident, const RunRequest &rq) {
        RunLayout L{};
        L.nwd = plan.nwin_local;
        L.shared = plan.shared != 0;
        L.n_points = n;
        L.nw = L.shared ? 1u : L.nwd;
        if (L.shared) n *= L.nwd;    // (window, point) pairs of all windows: one set of entries over one bucket set
        L.glv = plan.glv != 0;       // half scalars: entry 2 i = (P_i, k1_i), entry 2 i + 1 = (phi(P_i), k2_i)
        if (L.glv && (L.shared || resident)) return refuse(L, "GLV plan over registered bases");
        if (L.glv) n *= 2;
        if (n >= ((size_t)1 << 31)) return refuse(L, "n must be < 2^31");
        L.n = n;
        L.fork_convert = !resident && L.n_points >= FORK_CONVERT_MIN;
        L.q = plan_geometry(num_cus, L.nw, n, plan.nbuckets, L.shared);
        if constexpr (COMBINE_WE) {
            const unsigned tail = options().reduce_tail.load(std::memory_order_relaxed);
            const bool can = rq.tail_mode != TAIL_LADDER && !rq.d_out && !rq.buckets_only && !L.shared && L.q.nblocks1 <= PLANE_BLOCKS;
            L.planes = can && (tail == 2 || (tail == 0 && rq.tail_mode == TAIL_AUTO && PLANES_AUTO &&
                                             options().reduce_shape.load(std::memory_order_relaxed) == 0));
        }
        L.plane_np = 7 + L.q.plane_h;
        if ((L.error = plan_sort(num_cus, plan, L))) return L;
        L.d16 = max_digit_code(plan) < 65536;
        plan_scratch(plan.nbuckets, resident, L);
        if (L.nw > HEAVY_MAX_WINDOWS) return refuse(L, "more than 256 windows in one pipeline run");
        return L;
    }
    static RunLayout refuse(RunLayout &L, const char *why) {
        L.error = why;
        return L;
    }
    // grouping geometry of the two-pass sort; returns the refusal or nullptr
    static const char *plan_sort(int num_cus, const WindowPlan &plan, RunLayout &L) {
        const size_t n = L.n;
        const uint32_t NB = plan.nbuckets;
        while ((1u << L.log2NB) < NB) ++L.log2NB;
        uint32_t log2n = 0;
        while (((size_t)1 << log2n) < n) ++log2n;
        L.lidx = log2n + 1;  // bits of (index << 1 | negate)
        // target partition population 2^part_log2 (measured, BN254 G1: 2^13 is best up to 2^21 points - more
        // workgroups for the fine pass; 2^15 from 2^24 on - 128-byte runs out of the coarse pass)
        L.part_log2 = GMSM_TUNE(PART_LOG2, log2n <= 21 ? 13 : log2n >= 24 ? 15 : 14);
        int fb = (int)L.part_log2 + (int)L.log2NB - (int)log2n;
        if (fb > (int)L.log2NB) fb = (int)L.log2NB;
        if (fb > 15) fb = 15;  // the fine pass keeps 2^fb counters in LDS (128 KiB): windows wider than 16 bits on few points
        if (fb < 0) fb = 0;
        if (fb + L.lidx > 32) fb = 32 - L.lidx;
        L.fbits = (uint32_t)fb;
        L.nparts = NB >> L.fbits;
        L.big_chunk = n > ((size_t)1 << 25) && (size_t)L.nparts * 8 + PART_CHUNK_BIG * 6 <= 152 * 1024;
        L.pchunk_len = L.big_chunk ? PART_CHUNK_BIG : PART_CHUNK;  // chunk = one LDS staging buffer
        L.pchunks = (uint32_t)((n + L.pchunk_len - 1) / L.pchunk_len);
        L.scatter_lds = (size_t)L.nparts * 8 + L.pchunk_len * 6;
        if (L.scatter_lds > 152 * 1024)  // 32-bit sort entries: bucket bits + index bits; reached beyond 2^27 points at c <= 17
            return plan.c > 17 ? "window width too large for this many points in one pipeline run (a run takes up to "
                                 "2^(44-c) points for c > 17): use a smaller c or split by point range"
                               : "more than 2^27 points in one pipeline run: split the window sums by point range "
                                 "and add the sets (gmsm_fold_window_sets); the MultiExp entries do this themselves";
        // staging slots of the fine pass: up to 96 KiB next to the 2^fbits counters; larger partitions go direct
        const size_t fine_cnt_bytes = (size_t)4 << L.fbits;
        L.stage_cap = fine_cnt_bytes >= 156 * 1024 ? 0u
                                                   : (uint32_t)std::min<size_t>(GMSM_TUNE(STAGE_CAP, L.part_log2 >= 15 ? 39000 : 24576),
                                                                                (156 * 1024 - fine_cnt_bytes) / 4);
        if (L.stage_cap > 40u * 1024u) return "window geometry: staging slots beyond the fine sort's registers";
        if (fine_cnt_bytes + (size_t)L.stage_cap * 4 > 160 * 1024)  // cannot happen with fb <= 15; a failed launch must not
            return "window geometry: fine-sort counters exceed the LDS";  // leave garbage for the next kernels
        // oversized partitions of the fine sort (k_part_rowscan lists them, k_heavy_* sort them): a window has at most
        // n / (stage_cap + 1) of them, and their sub-runs of HEAVY_SUB references number at most n / HEAVY_SUB + that
        L.hcap = (uint32_t)std::min<size_t>(L.nparts, n / ((size_t)L.stage_cap + 1) + 1);
        L.scap = (uint32_t)(n / HEAVY_SUB) + L.hcap;
        // workgroups of the heavy kernels (the sub-runs of all windows are taken round-robin): the chip twice over
        L.heavy_wg = (uint32_t)std::min<size_t>((size_t)2 * num_cus, std::max<size_t>((size_t)L.nw * L.scap, 1));
        return nullptr;
    }
    static void plan_scratch(uint32_t NB, bool resident, RunLayout &L) {
        const size_t nw = L.nw, n = L.n, tot_thr = nw * L.q.tpw;
        L.digits = nw * n * (L.d16 ? 2 : 4);
        L.sorted = L.parted = nw * n * 4;
        L.starts = nw * (NB + 1) * 4;
        L.buckets = nw * NB * REC;
        L.partials = partials_bytes(L.q, L.nw, L.planes);
        L.red_pre = red_pre_bytes(L.q, L.nw);
        L.totals = (size_t)L.nwd * sizeof(Ext);
        L.pinned = (size_t)L.nwd * (L.planes ? L.plane_np : 1u) * sizeof(Ext);
        L.blockhist = nw * L.pchunks * L.nparts * 4;
        L.counts = nw * (2 * L.nparts + 1) * 4;
        L.seg_partials = tot_thr * 2 * REC;
        L.seg_flags = L.seg_bucket = tot_thr * 4;
        // long-chain list of the fixup (the fix-up kernels append pieces of LONG_PIECE links, k_fixup_long consumes): one counter
        // (slot of the first window; k_part_rowscan zeroes it) + the items: chains have more than FIX_MAXWALK followers.
        // (The factor 2 dates from an experiment that gave each of two window groups its own half; it only sizes the buffer.)
        L.list_cap = 2 * (tot_thr / FIX_MAXWALK + tot_thr / LONG_PIECE + nw + 16);
        L.seg_lvl = nw * 4 + 16 + L.list_cap * sizeof(LongChain);
        L.piece_sums_off = ((L.list_cap * 4 + 15) / 16) * 16;
        L.long_pieces = L.piece_sums_off + L.list_cap * REC;
        L.hparts_bytes = ((nw * L.hcap * sizeof(HeavyPart) + 15) / 16) * 16;
        L.hcount_bytes = ((nw * 8 + 4 + 15) / 16) * 16;
        L.heavy = L.hparts_bytes + L.hcount_bytes + (nw * L.scap << L.fbits) * 4;
        L.upoints = resident ? 0 : (L.glv ? 2 : 1) * L.n_points * AFF_BYTES;
    }
    // gmsm_debug_run_layout: the layout as integers, in the order of tests/golden/pipeline_layout.json's "fields"
    static constexpr int LAYOUT_WORDS = GMSM_RUN_LAYOUT_WORDS;
    static void flatten(int num_cus, const RunLayout &L, uint64_t out[LAYOUT_WORDS]) {
        const Geometry &q = L.q;
        const uint64_t v[LAYOUT_WORDS] = {
            L.nw, L.nwd, L.n, L.d16, q.seg, q.tpw, q.log2L, q.nblocks1, q.log2span, q.nblocks2, q.T, q.plane_h, L.planes, L.plane_np,
            L.log2NB, L.lidx, L.part_log2, L.fbits, L.nparts, L.big_chunk, L.pchunk_len, L.pchunks, L.scatter_lds, L.stage_cap, L.hcap,
            L.scap, L.heavy_wg, L.list_cap, use_combine_we(num_cus, q.nblocks1 * L.nw) ? 2u : 1u,
            reduce2_active(q.nblocks2 ? q.nblocks2 : q.nblocks1),
            L.digits, L.sorted, L.parted, L.starts, L.buckets, L.partials, L.red_pre, L.totals, L.pinned, L.blockhist, L.counts,
            L.seg_partials, L.seg_flags, L.seg_bucket, L.seg_lvl, L.long_pieces, L.heavy, L.upoints, L.piece_sums_off, L.hparts_bytes,
            L.hcount_bytes};
        memcpy(out, v, sizeof v);
    }

    // ------------------------------------------------------------------ what is reserved
    // The scratch of one run, carved: every pointer lies in a buffer of `ws`.
    struct Buffers {
        void *digits;
        uint32_t *sorted, *parted, *starts, *seg_flags, *seg_bucket;
        char *buckets, *seg_partials;
        uint32_t *long_flag;   // [nw] counters of the long-chain list, [0] is used
        LongChain *long_list;
        uint32_t *piece_done;
        void *piece_sums;
        HeavyPart *hparts;
        uint32_t *hcount, *subhist, *bh, *part_base, *part_pop;
    };
    static int reserve(Workspace &ws, const RunLayout &L, Buffers &b) {
        const struct {
            DeviceBuffer &buf;
            size_t bytes;
        } need[] = {{ws.digits, L.digits}, {ws.sorted, L.sorted}, {ws.parted, L.parted}, {ws.starts, L.starts}, {ws.buckets, L.buckets},
                    {ws.partials, L.partials}, {ws.red_pre, L.red_pre}, {ws.totals, L.totals}, {ws.blockhist, L.blockhist},
                    {ws.counts, L.counts}, {ws.seg_partials, L.seg_partials}, {ws.seg_flags, L.seg_flags}, {ws.seg_bucket, L.seg_bucket},
                    {ws.seg_lvl, L.seg_lvl}, {ws.long_pieces, L.long_pieces}, {ws.heavy, L.heavy}, {ws.upoints, L.upoints}};
        int rc;
        for (const auto &e : need)
            if ((rc = e.buf.ensure(e.bytes))) return rc;
        if ((rc = ws.ensure_pinned(L.pinned))) return rc;
        b.digits = ws.digits.ptr;
        b.sorted = (uint32_t *)ws.sorted.ptr, b.parted = (uint32_t *)ws.parted.ptr, b.starts = (uint32_t *)ws.starts.ptr;
        b.seg_flags = (uint32_t *)ws.seg_flags.ptr, b.seg_bucket = (uint32_t *)ws.seg_bucket.ptr;
        b.buckets = (char *)ws.buckets.ptr, b.seg_partials = (char *)ws.seg_partials.ptr;
        b.long_flag = (uint32_t *)ws.seg_lvl.ptr;
        b.long_list = (LongChain *)((char *)ws.seg_lvl.ptr + (((size_t)L.nw * 4 + 15) / 16) * 16);
        b.piece_done = (uint32_t *)ws.long_pieces.ptr;
        b.piece_sums = (char *)ws.long_pieces.ptr + L.piece_sums_off;
        b.hparts = (HeavyPart *)ws.heavy.ptr;
        b.hcount = (uint32_t *)((char *)ws.heavy.ptr + L.hparts_bytes);
        b.subhist = (uint32_t *)((char *)ws.heavy.ptr + L.hparts_bytes + L.hcount_bytes);
        b.bh = (uint32_t *)ws.blockhist.ptr, b.part_base = (uint32_t *)ws.counts.ptr;
        b.part_pop = b.part_base + (size_t)L.nw * (L.nparts + 1);
        return GMSM_OK;
    }
    // Kernels of the pipeline that need more than the default 64 KiB of dynamic LDS (once per kernel and device).
    static int allow_pipeline_lds(Context &ctx, bool planes) {
        int rc;
        if ((rc = ctx.allow_lds((const void *)k_part_hist<uint16_t>, 160 * 1024))) return rc;
        if ((rc = ctx.allow_lds((const void *)k_part_hist<uint32_t>, 160 * 1024))) return rc;
        if ((rc = ctx.allow_lds((const void *)k_part_scatter<uint16_t, PART_CHUNK>, 152 * 1024))) return rc;
        if ((rc = ctx.allow_lds((const void *)k_part_scatter<uint32_t, PART_CHUNK>, 152 * 1024))) return rc;
        if ((rc = ctx.allow_lds((const void *)k_part_scatter<uint16_t, PART_CHUNK_BIG>, 152 * 1024))) return rc;
        if ((rc = ctx.allow_lds((const void *)k_part_scatter<uint32_t, PART_CHUNK_BIG>, 152 * 1024))) return rc;
        if ((rc = ctx.allow_lds((const void *)k_fine_sort<24>, 160 * 1024))) return rc;
        if ((rc = ctx.allow_lds((const void *)k_fine_sort<40>, 160 * 1024))) return rc;
        if ((rc = ctx.allow_lds((const void *)k_heavy_hist, 128 * 1024))) return rc;
        if ((rc = ctx.allow_lds((const void *)k_heavy_scan, 128 * 1024))) return rc;
        if ((rc = ctx.allow_lds((const void *)k_heavy_place, 128 * 1024))) return rc;
        if ((rc = ctx.allow_lds((const void *)k_fixup_long<U>, (int)(128 * sizeof(QRec<U>))))) return rc;
        if constexpr (FIXUP_QUAD)
            if ((rc = ctx.allow_lds((const void *)k_fixup_seg_q<U>, (int)(128 * sizeof(QRec<U>))))) return rc;
        if ((rc = ctx.allow_lds((const void *)k_combine_q<U, true, COMBINE_N>, (int)((2 * COMBINE_N + 1) * sizeof(QRec<U>))))) return rc;
        if constexpr (COMBINE_WE)
            if ((rc = ctx.allow_lds((const void *)k_combine_we<U, true>, (int)((2 * COMBINE_N + 1) * sizeof(QRec<U>))))) return rc;
        if constexpr (SERIAL_QUAD)
            if ((rc = ctx.allow_lds((const void *)k_reduce_serial_q<U, SERIAL_Q_QUADS>, (int)(3 * SERIAL_Q_QUADS * sizeof(QRec<U>))))) return rc;
        if ((rc = ctx.allow_lds((const void *)k_reduce2_q<U, true>, (int)(2 * RED2_TPB * sizeof(QRec<U>))))) return rc;
        if constexpr (COMBINE_WE) {
            if (planes) {
                if ((rc = ctx.allow_lds((const void *)k_combine_we<U, true, true>, (int)((2 * COMBINE_N + 1) * sizeof(QRec<U>))))) return rc;
                if ((rc = ctx.allow_lds((const void *)k_plane_sums<U, true>, (int)(PLANE_BLOCKS * sizeof(QRec<U>))))) return rc;
            }
        }
        return GMSM_OK;
    }

    // ------------------------------------------------------------------ what is launched
    // k_decompose for this plan: the unrolled kernel of the plan's width when it is one of the window table's
    // (preferred_c), the generic one otherwise (forced and test widths). d16: uint16 digit codes.
    static void launch_decompose(const void *d_scalars, size_t n, const WindowPlan &plan, bool d16, void *digits,
                                 const uint8_t *skip, hipStream_t stream) {
        const dim3 grid((unsigned)((n + 255) / 256)), block(256);
        if (plan.glv) {  // half scalars: digits[k][2 n] (glv_width_built() lists the widths)
#define GMSM_DECOMPOSE_GLV(CC)                                                                                                  \
    case CC:                                                                                                                    \
        if (d16) hipLaunchKernelGGL((k_decompose_glv<FrP, uint16_t, CC>), grid, block, 0, stream, (const uint32_t *)d_scalars, n, \
                                    plan, (uint16_t *)digits, skip);                                                             \
        else hipLaunchKernelGGL((k_decompose_glv<FrP, uint32_t, CC>), grid, block, 0, stream, (const uint32_t *)d_scalars, n,     \
                                plan, (uint32_t *)digits, skip);                                                                 \
        return;
            switch (plan.c) {
                GMSM_DECOMPOSE_GLV(10) GMSM_DECOMPOSE_GLV(11) GMSM_DECOMPOSE_GLV(12) GMSM_DECOMPOSE_GLV(13) GMSM_DECOMPOSE_GLV(14)
                GMSM_DECOMPOSE_GLV(15) GMSM_DECOMPOSE_GLV(16) GMSM_DECOMPOSE_GLV(17) GMSM_DECOMPOSE_GLV(18) GMSM_DECOMPOSE_GLV(20)
                default: return;  // never planned (glv_width_built)
            }
#undef GMSM_DECOMPOSE_GLV
        }
#define GMSM_DECOMPOSE_C(CC)                                                                                                \
    case CC:                                                                                                                \
        if (d16) hipLaunchKernelGGL((k_decompose_c<FrP, uint16_t, CC>), grid, block, 0, stream, (const uint32_t *)d_scalars, n,  \
                                    plan, (uint16_t *)digits, skip);                                                         \
        else hipLaunchKernelGGL((k_decompose_c<FrP, uint32_t, CC>), grid, block, 0, stream, (const uint32_t *)d_scalars, n,      \
                                plan, (uint32_t *)digits, skip);                                                             \
        return;
        switch (plan.c) {
            GMSM_DECOMPOSE_C(8) GMSM_DECOMPOSE_C(9) GMSM_DECOMPOSE_C(10) GMSM_DECOMPOSE_C(12) GMSM_DECOMPOSE_C(13)
            GMSM_DECOMPOSE_C(14) GMSM_DECOMPOSE_C(15) GMSM_DECOMPOSE_C(16) GMSM_DECOMPOSE_C(17) GMSM_DECOMPOSE_C(18)
            GMSM_DECOMPOSE_C(20)
            default: break;
        }
#undef GMSM_DECOMPOSE_C
        if (d16)
            hipLaunchKernelGGL((k_decompose<FrP, uint16_t>), grid, block, 0, stream, (const uint32_t *)d_scalars, n, plan,
                               (uint16_t *)digits, skip);
        else
            hipLaunchKernelGGL((k_decompose<FrP, uint32_t>), grid, block, 0, stream, (const uint32_t *)d_scalars, n, plan,
                               (uint32_t *)digits, skip);
    }

    // Launches every kernel of one pipeline run and queues the copy of the window totals into ws.pinned; does not wait.
    // d_points: Go-layout affine bases on the device, or nullptr when `resident` (bases already rewritten into the lazy
    // domain by register_bases) is given. `stream` carries the call (inputs are ready there; the totals are complete
    // there). All scratch comes from `ws`, so two workspaces can be in flight at once.
    // (Cutting the windows of a call into two groups, so that the fix-up and reduction of one ran beside the accumulation
    // of the other, was measured in round 2 and again in round 5 - profiles/r02_split_ab.log, profiles/r05_split_groups.log:
    // no gain either time, and the code is gone.)
    static int enqueue_window_sums(Context &ctx, Workspace &ws, const void *d_points, const void *d_scalars, size_t n,
                                   const WindowPlan &plan, hipStream_t stream, const ResidentBases *resident,
                                   const RunRequest &rq = RunRequest{}) {
        const uint32_t nwd = plan.nwin_local;
        ws.pending_timed = false;
        ws.plane_np = 0;
        if (nwd == 0) return GMSM_OK;
        // window tables: the (window, point) pairs of all windows form ONE set of entries over one bucket set
        const bool shared = plan.shared != 0;
        if (shared && !(resident && resident->tab_c.load() == plan.c && plan.win_first == 0 && plan.win_stride == 1))
            return fail(GMSM_ERR_ARG, "shared-bucket plan without matching window tables");
        if (shared && n) g_table_runs.fetch_add(1, std::memory_order_relaxed);
        if (ws.uncollected) {  // stage events of an enqueue-only call (nobody waited for it): pick them up now
            if (ws.timed && hipEventQuery(ws.events[ws.timed_level == 2 ? T_FIXUP : T_END]) == hipSuccess) StageTimer::collect(ws);
            ws.uncollected = false;
        }
        // The workspace may still be in use by work enqueued earlier on another stream: order behind it.
        int rc;
        if ((rc = begin_use(ws, stream))) return rc;
        if (n == 0) return enqueue_infinities(ws, nwd, rq.d_out, stream);
        const RunLayout L = plan_run(ctx.num_cus, plan, n, resident != nullptr, rq);
        if (L.error) return fail(GMSM_ERR_ARG, L.error);
        Buffers b;
        if ((rc = reserve(ws, L, b))) return rc;
        if ((rc = allow_pipeline_lds(ctx, L.planes))) return rc;
        // Stage times cover single-run calls: the ranges of a multi-range call (buckets_only) reuse a workspace's events
        // before anybody could read them, and their merges and the one reduction run on another stream - such calls are
        // left out of the profile instead of being reported with two of their ranges and no reduction.
        StageTimer timer(ws, /*enabled=*/!rq.buckets_only || rq.time_range);
        ws.timed = timer.on;
        const void *upoints = nullptr;
        if ((rc = stage_inputs(ws, L, b, plan, d_points, d_scalars, resident, rq.resident_offset, stream, timer, &upoints))) return rc;
        stage_sort(ctx.num_cus, L, b, plan.nbuckets, stream, timer);
        if ((rc = stage_accumulate(ws, L, b, plan.nbuckets, upoints, resident, stream, timer))) return rc;
        stage_fixup(ctx.num_cus, L, b, plan.nbuckets, stream, timer);
        stage_reduce(ctx.num_cus, ws, L, b, plan.nbuckets, rq.buckets_only, stream, timer);
        return stage_result(ws, L, rq, stream, timer);
    }
    // a run over no points: every total is the point at infinity
    static int enqueue_infinities(Workspace &ws, uint32_t nwd, void *d_out, hipStream_t stream) {
        int rc0 = ws.ensure_pinned((size_t)nwd * sizeof(Ext));
        if (rc0) return rc0;
        if (d_out) HIP_TRY(hipStreamSynchronize(stream));  // an earlier copy out of ws.pinned may be in flight
        for (uint32_t k = 0; k < nwd; ++k) ((Ext *)ws.pinned)[k] = Ext::infinity();
        if (d_out) {
            HIP_TRY(hipMemcpyAsync(d_out, ws.pinned, (size_t)nwd * sizeof(Ext), hipMemcpyHostToDevice, stream));
            HIP_TRY(hipStreamSynchronize(stream));
        }
        return GMSM_OK;
    }

    // ---- 0. inputs: rewrite the bases into the lazy Montgomery domain + infinity flags (unless registered earlier),
    // signed-digit decomposition of every scalar. *upoints: the rewritten bases the accumulation reads.
    static int stage_inputs(Workspace &ws, const RunLayout &L, const Buffers &b, const WindowPlan &plan, const void *d_points,
                            const void *d_scalars, const ResidentBases *resident, size_t resident_offset, hipStream_t stream,
                            StageTimer &timer, const void **upoints) {
        timer.mark(T_DECOMPOSE, stream);
        const uint8_t *skip = nullptr;
        const size_t n_points = L.n_points;
        if (resident) {
            *upoints = (const char *)(L.shared ? resident->tables.ptr : resident->upoints.ptr) + resident_offset * AFF_BYTES;
            skip = (const uint8_t *)resident->skip.ptr + resident_offset;
        } else {
            // Round 4: the rewrite of the bases runs on a stream of its own BESIDE the scalar pipeline (decomposition and
            // the two sort passes touch only the scalars; those kernels are bound by LDS atomics and latency, the rewrite
            // by HBM) and joins before the accumulation. Infinity points are recognised by the accumulation from the
            // rewritten record (uaffine_is_infinity), so the decomposition needs no flags from here. 2^20: 36 us off the
            // critical path, 2^24: 0.44 ms. Small calls keep the single stream (two events cost more than they hide).
            const bool forked = L.fork_convert;
            int rc;
            if (forked && (rc = ws.side_stream(ws.cstream))) return rc;
            hipStream_t cs = forked ? ws.cstream : stream;
            if (forked) {
                HIP_TRY(hipEventRecord(ws.ev_fork, stream));
                HIP_TRY(hipStreamWaitEvent(cs, ws.ev_fork, 0));
            }
            if (L.glv)
                hipLaunchKernelGGL((k_convert_points_glv<U, Consts>), dim3((unsigned)((n_points + 255) / 256)), dim3(256), 0,
                                   cs, d_points, n_points, ws.upoints.ptr);
            else
                hipLaunchKernelGGL((k_convert_points<U>), dim3((unsigned)((n_points + 255) / 256)), dim3(256), 0,
                                   cs, d_points, n_points, ws.upoints.ptr, (uint8_t *)nullptr);
            if (forked) {
                ws.conv_pending = true;  // until the join is enqueued (stage_accumulate; an error return in between leaves cstream running)
                HIP_TRY(hipEventRecord(ws.ev_conv, cs));
            }
            *upoints = ws.upoints.ptr;
        }
        // (A decomposition fused with the coarse histogram was measured and dropped: one workgroup per 16 K-scalar chunk
        // leaves 3/4 of the CUs idle at 2^20, and at 2^24 it only breaks even.)
        // (shared: digits[w][i] of the n_points scalars, read from here on as one window of nwd * n_points entries)
        launch_decompose(d_scalars, n_points, plan, L.d16, b.digits, skip, stream);
        return GMSM_OK;
    }

    // ---- 1. group the point references of every window by bucket
    static void stage_sort(int num_cus, const RunLayout &L, const Buffers &b, uint32_t NB, hipStream_t stream, StageTimer &timer) {
        const size_t n = L.n, pchunk_len = L.pchunk_len, scatter_lds = L.scatter_lds;
        const uint32_t nw = L.nw, nparts = L.nparts, fbits = L.fbits, lidx = L.lidx, pchunks = L.pchunks, stage_cap = L.stage_cap;
        const uint32_t hcap = L.hcap, scap = L.scap;
        timer.mark(T_HIST, stream);
        if (L.d16)
            hipLaunchKernelGGL(k_part_hist<uint16_t>, dim3(pchunks, nw), dim3(1024), (size_t)nparts * 4, stream,
                               (const uint16_t *)b.digits, n, nparts, fbits, pchunk_len, b.bh);
        else
            hipLaunchKernelGGL(k_part_hist<uint32_t>, dim3(pchunks, nw), dim3(1024), (size_t)nparts * 4, stream,
                               (const uint32_t *)b.digits, n, nparts, fbits, pchunk_len, b.bh);
        timer.mark(T_SCAN, stream);
        if ((size_t)((nparts + 31) / 32) * nw < (size_t)num_cus && pchunks >= 256)
            hipLaunchKernelGGL(k_part_colscan<32>, dim3((nparts + 31) / 32, nw), dim3(1024), 0, stream, b.bh, pchunks, nparts, b.part_pop, b.hcount + 2 * nw);
        else
            hipLaunchKernelGGL(k_part_colscan<8>, dim3((nparts + 31) / 32, nw), dim3(256), 0, stream, b.bh, pchunks, nparts, b.part_pop, b.hcount + 2 * nw);
        hipLaunchKernelGGL(k_part_rowscan, dim3(nw), dim3(1024), 0, stream, b.part_pop, nparts, b.part_base, b.long_flag, stage_cap, b.hparts,
                           b.hcount, hcap);
        timer.mark(T_SCATTER, stream);
        {
            const dim3 grid(pchunks, nw), block(1024);
#define GMSM_SCATTER(D, CH)                                                                                                \
    hipLaunchKernelGGL((k_part_scatter<D, CH>), grid, block, scatter_lds, stream, (const D *)b.digits, n, nparts, fbits, lidx, \
                       pchunk_len, b.bh, b.part_base, b.parted)
            if (L.d16 && !L.big_chunk) GMSM_SCATTER(uint16_t, PART_CHUNK);
            else if (L.d16) GMSM_SCATTER(uint16_t, PART_CHUNK_BIG);
            else if (!L.big_chunk) GMSM_SCATTER(uint32_t, PART_CHUNK);
            else GMSM_SCATTER(uint32_t, PART_CHUNK_BIG);
#undef GMSM_SCATTER
        }
        // the partition's references stay in registers between the two passes: 24 per thread (stage_cap <= 24576), else 40
        if (stage_cap <= 24u * 1024u)
            hipLaunchKernelGGL(k_fine_sort<24>, dim3(nparts, nw), dim3(1024), ((size_t)4 << fbits) + (size_t)stage_cap * 4, stream,
                               b.parted, n, NB, fbits, lidx, b.part_base, b.sorted, b.starts, stage_cap);
        else
            hipLaunchKernelGGL(k_fine_sort<40>, dim3(nparts, nw), dim3(1024), ((size_t)4 << fbits) + (size_t)stage_cap * 4, stream,
                               b.parted, n, NB, fbits, lidx, b.part_base, b.sorted, b.starts, stage_cap);
        // partitions beyond the staging slots (crowded buckets, narrow top windows): sorted by many workgroups each. A run of at
        // most stage_cap entries per window cannot have one: no launches (14 us of a 0.4 ms call)
        if (n > stage_cap) {
            hipLaunchKernelGGL(k_heavy_hist, dim3(L.heavy_wg), dim3(1024), (size_t)4 << fbits, stream, b.parted, n, nw, nparts, fbits, lidx,
                               b.part_base, (const HeavyPart *)b.hparts, (const uint32_t *)b.hcount, hcap, scap, b.subhist);
            hipLaunchKernelGGL(k_heavy_scan, dim3(std::min<uint32_t>(hcap, 64u), nw), dim3(1024), (size_t)4 << fbits, stream, nparts, NB, fbits,
                               b.part_base, (const HeavyPart *)b.hparts, (const uint32_t *)b.hcount, hcap, scap, b.subhist, b.starts);
            hipLaunchKernelGGL(k_heavy_place, dim3(L.heavy_wg), dim3(1024), (size_t)4 << fbits, stream, b.parted, n, nw, nparts, fbits, lidx,
                               b.part_base, (const HeavyPart *)b.hparts, (const uint32_t *)b.hcount, hcap, scap, (const uint32_t *)b.subhist, b.sorted);
        }
    }

    // ---- 2. bucket accumulation, once the rewritten bases are complete
    static int stage_accumulate(Workspace &ws, const RunLayout &L, const Buffers &b, uint32_t NB, const void *upoints,
                                const ResidentBases *resident, hipStream_t stream, StageTimer &timer) {
        const Geometry &q = L.q;
        if (L.fork_convert) {
            HIP_TRY(hipStreamWaitEvent(stream, ws.ev_conv, 0));
            ws.conv_pending = false;
        }
        timer.mark(T_ACCUMULATE, stream);
        if (L.shared)
            hipLaunchKernelGGL((k_accumulate_seg<U, true>), dim3((q.tpw + 255) / 256, L.nw), dim3(256), 0, stream, upoints, L.n, NB,
                               q.seg, (const uint32_t *)b.starts, (const uint32_t *)b.sorted, b.buckets, b.seg_partials, b.seg_flags, b.seg_bucket,
                               q.tpw, (uint32_t)L.n_points, (uint32_t)resident->n);
        else
            hipLaunchKernelGGL((k_accumulate_seg<U, false>), dim3((q.tpw + 255) / 256, L.nw), dim3(256), 0, stream, upoints, L.n, NB,
                               q.seg, (const uint32_t *)b.starts, (const uint32_t *)b.sorted, b.buckets, b.seg_partials, b.seg_flags, b.seg_bucket,
                               q.tpw, 0u, 0u);
        return GMSM_OK;
    }

    // ---- 3. fix-up: close the buckets whose entries were split over several accumulation threads
    static void stage_fixup(int num_cus, const RunLayout &L, const Buffers &b, uint32_t NB, hipStream_t stream, StageTimer &timer) {
        const Geometry &q = L.q;
        const uint32_t nw = L.nw;
        const uint32_t *starts = b.starts, *flags = b.seg_flags, *pb = b.seg_bucket;
        timer.mark(T_FIXUP, stream);
        if (L.shared && L.n / NB >= 2 * (size_t)q.seg)  // buckets of several threads' worth of entries (dense chains): one thread per bucket
            hipLaunchKernelGGL((k_fixup_bucket<OpsSerial>), dim3((NB + 255) / 256, nw), dim3(256), 0, stream, NB, starts, q.seg,
                               (const void *)b.seg_partials, q.tpw, (void *)b.buckets, b.long_flag, b.long_list, b.piece_done, FIX_MAXWALK);
        else if constexpr (FIXUP_QUAD)
            hipLaunchKernelGGL((k_fixup_seg_q<U>), dim3((q.tpw + 63) / 64, nw), dim3(256), 128 * sizeof(QRec<U>), stream, NB,
                               (const void *)b.seg_partials, flags, pb, q.tpw, (void *)b.buckets, b.long_flag, b.long_list, b.piece_done, FIX_MAXWALK, starts, q.seg);
        else
            hipLaunchKernelGGL((k_fixup_seg<OpsSerial>), dim3((q.tpw + 255) / 256, nw), dim3(256), 0, stream, NB, b.seg_partials, flags, pb,
                               q.tpw, b.buckets, b.long_flag, b.long_list, b.piece_done, FIX_MAXWALK, starts, q.seg);
        hipLaunchKernelGGL((k_fixup_long<U>), dim3(2 * num_cus), dim3(256), 128 * sizeof(QRec<U>), stream, NB, b.seg_partials, pb, q.tpw,
                           b.buckets, (const uint32_t *)b.long_flag, (const LongChain *)b.long_list, b.piece_done, b.piece_sums, starts, q.seg);
    }

    // ---- 4. bucket reduction -> window totals (empty buckets are never written: the reduction consults starts[])
    static void stage_reduce(int num_cus, Workspace &ws, const RunLayout &L, const Buffers &b, uint32_t NB, bool buckets_only,
                             hipStream_t stream, StageTimer &timer) {
        timer.mark(T_REDUCE, stream);
        if (!buckets_only) enqueue_reduce_kernels(num_cus, ws, L.q, b.buckets, b.starts, L.nw, NB, stream, L.planes);
    }

    // ---- 5. result: the totals of windows without a bucket set, the copy (or the note of what ws.pinned holds)
    static int stage_result(Workspace &ws, const RunLayout &L, const RunRequest &rq, hipStream_t stream, StageTimer &timer) {
        const uint32_t nw = L.nw, nwd = L.nwd;
        if (!rq.buckets_only && nwd > nw)
            hipLaunchKernelGGL((k_fill_infinity<Ext>), dim3((nwd - nw + 63) / 64), dim3(64), 0, stream, ws.totals.ptr, nw, nwd - nw);
        timer.mark(T_END, stream);
        HIP_TRY(hipGetLastError());
        if (L.planes) {  // k_plane_sums wrote ws.pinned itself: nothing to copy
            ws.plane_np = L.plane_np;
            ws.plane_log2L = L.q.log2L;
            g_plane_runs.fetch_add(1, std::memory_order_relaxed);
        } else if (!rq.buckets_only) {
            if (rq.d_out)
                HIP_TRY(hipMemcpyAsync(rq.d_out, ws.totals.ptr, (size_t)nwd * sizeof(Ext), hipMemcpyDeviceToDevice, stream));
            else
                HIP_TRY(hipMemcpyAsync(ws.pinned, ws.totals.ptr, (size_t)nwd * sizeof(Ext), hipMemcpyDeviceToHost, stream));
        }
        int rc;
        if ((rc = end_use(ws, stream))) return rc;
        ws.pending_timed = timer.on;
        return GMSM_OK;
    }

    // The three kernels of the bucket reduction: buckets (nw x NB lazy records; starts == nullptr: every record is
    // stored, infinity as zz = 0) -> ws.totals, or (planes) the plane sums -> ws.pinned. Scratch: ws.red_pre, ws.partials.
    static void enqueue_reduce_kernels(int num_cus, Workspace &ws, const Geometry &q, const void *buckets, const uint32_t *starts,
                                       uint32_t nw, uint32_t NB, hipStream_t stream, bool planes = false) {
        void *red_pre = ws.red_pre.ptr, *partials = ws.partials.ptr;
        const uint32_t T = q.T;
        // level 1 leaves S_blk already multiplied by the width of the level-2 spans (an otherwise idle quad doubles it
        // log2span times while the trees run): level 2 then has no serial doubling tail
        const uint32_t prescale = q.log2span;
        if constexpr (SERIAL_QUAD)
            hipLaunchKernelGGL((k_reduce_serial_q<U, SERIAL_Q_QUADS>), dim3((T + SERIAL_Q_QUADS - 1) / SERIAL_Q_QUADS, nw), dim3(4 * SERIAL_Q_QUADS),
                               3 * SERIAL_Q_QUADS * sizeof(QRec<U>), stream, buckets, NB, q.log2L, T, starts, red_pre);
        else
            hipLaunchKernelGGL((k_reduce_serial<OpsSerial>), dim3((T + 255) / 256, nw), dim3(256), 0, stream, buckets, NB,
                               q.log2L, T, starts, red_pre);
        if constexpr (COMBINE_WE) {
            if (planes) {  // GMSM_OPT_REDUCE_TAIL: sums only, the host fold applies the weights (fold_planes)
                const uint32_t h = q.plane_h;
                const uint32_t quads = std::min(64u, std::max(16u, (1u << h) / 2));  // a step has at most 2^h / 2 additions
                hipLaunchKernelGGL((k_combine_we<U, true, true>), dim3(q.nblocks1, nw), dim3(4 * COMBINE_N),
                                   (2 * COMBINE_N + 1) * sizeof(QRec<U>), stream, q.log2L, ws.partials.ptr, 0u, (const void *)red_pre, T);
                hipLaunchKernelGGL((k_plane_sums<U, true>), dim3(nw, 8), dim3(4 * quads), ((size_t)1 << h) * sizeof(QRec<U>), stream,
                                   (const void *)ws.partials.ptr, q.nblocks1, h, ws.pinned);
                return;
            }
        }
        // one combine level: `pairs` (S, W) pairs per window, each the sum of 2^l2 buckets (S prescaled by the caller's
        // factor when l2 == 0) -> `blocks` pairs per window
        const auto combine = [&](const void *in, uint32_t pairs, void *out, uint32_t blocks, uint32_t l2, uint32_t pre) {
            if constexpr (COMBINE_WE) {
                if (use_combine_we(num_cus, blocks * nw)) {
                    hipLaunchKernelGGL((k_combine_we<U, true>), dim3(blocks, nw), dim3(4 * COMBINE_N),
                                       (2 * COMBINE_N + 1) * sizeof(QRec<U>), stream, l2, out, pre, in, pairs);
                    return;
                }
            }
            hipLaunchKernelGGL((k_combine_q<U, true, COMBINE_N>), dim3(blocks, nw), dim3(4 * COMBINE_N),
                               (2 * COMBINE_N + 1) * sizeof(QRec<U>), stream, l2, out, pre, in, pairs);
        };
        combine(red_pre, T, partials, q.nblocks1, q.log2L, prescale);
        const void *last = partials;
        uint32_t nlast = q.nblocks1, rest = q.log2span - prescale;
        if (q.nblocks2) {
            // second combine: its input pairs carry S already multiplied by their own span (the prescale above), so the
            // pairs count as single buckets (L = 1); its S_blk is doubled log2 N more times for the last level
            void *out2 = (char *)partials + (size_t)nw * q.nblocks1 * 2 * REC;
            uint32_t lgN = 0;
            for (size_t t = COMBINE_N; t > 1; t >>= 1) ++lgN;
            combine(partials, q.nblocks1, out2, q.nblocks2, 0, lgN);
            last = out2;
            nlast = q.nblocks2;
            rest = 0;
        }
        const uint32_t active = reduce2_active(nlast);
        hipLaunchKernelGGL((k_reduce2_q<U, true>), dim3(nw), dim3(4 * active), 2 * active * sizeof(QRec<U>), stream, last, nlast,
                           rest, active, ws.totals.ptr);
    }

    // The reduction alone, over bucket sums that a multi-range call has merged (every record stored): totals -> ws.pinned.
    static int enqueue_reduce(Context &ctx, Workspace &ws, const void *buckets, const WindowPlan &plan, size_t n_for_geometry,
                              hipStream_t stream) {
        const uint32_t nw = bucket_sets(plan), nwd = plan.nwin_local, NB = plan.nbuckets;
        const Geometry q = plan_geometry(ctx.num_cus, nw, n_for_geometry, NB);
        int rc;
        ws.plane_np = 0;
        if ((rc = ws.partials.ensure(partials_bytes(q, nw, false)))) return rc;
        if ((rc = ws.red_pre.ensure(red_pre_bytes(q, nw)))) return rc;
        if ((rc = ws.totals.ensure((size_t)nwd * sizeof(Ext)))) return rc;
        if ((rc = ws.ensure_pinned((size_t)nwd * sizeof(Ext)))) return rc;
        if ((rc = allow_pipeline_lds(ctx, false))) return rc;
        enqueue_reduce_kernels(ctx.num_cus, ws, q, buckets, nullptr, nw, NB, stream);
        if (nwd > nw)
            hipLaunchKernelGGL((k_fill_infinity<Ext>), dim3((nwd - nw + 63) / 64), dim3(64), 0, stream, ws.totals.ptr, nw, nwd - nw);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(ws.pinned, ws.totals.ptr, (size_t)nwd * sizeof(Ext), hipMemcpyDeviceToHost, stream));
        return GMSM_OK;
    }

    // ------------------------------------------------------------------ what the caller collects
    // Waits for the pipeline enqueued on `stream` and hands out the window totals (pinned buffer -> host_xyzz).
    static int collect_window_sums(Workspace &ws, hipStream_t stream, uint32_t nw, Ext *host_xyzz) {
        if (nw == 0) return GMSM_OK;
        HIP_TRY(wait_stream(stream));
        if (ws.pending_timed) StageTimer::collect(ws);
        ws.pending_timed = false;
        if (ws.plane_np) {  // plane sums: every window's own Horner walk
            const Ext *planes = (const Ext *)ws.pinned;
            for (uint32_t w = 0; w < nw; ++w) {
                const J j = fold_planes(planes + (size_t)w * ws.plane_np, 0, 1, ws.plane_log2L, ws.plane_np - 7);
                host_xyzz[w] = j.z.is_zero() ? Ext::infinity() : xyzz_from_jac(j);
            }
            return GMSM_OK;
        }
        memcpy(host_xyzz, ws.pinned, (size_t)nw * sizeof(Ext));
        return GMSM_OK;
    }
    // ... and folds them: msmReduceChunk over nwin window totals, or over their plane sums
    static int collect_folded(Workspace &ws, hipStream_t stream, unsigned c, uint32_t nwin, J *out) {
        if (ws.plane_np) {
            HIP_TRY(wait_stream(stream));
            if (ws.pending_timed) StageTimer::collect(ws);
            ws.pending_timed = false;
            *out = fold_planes((const Ext *)ws.pinned, c, nwin, ws.plane_log2L, ws.plane_np - 7);
            return GMSM_OK;
        }
        std::vector<Ext> totals(nwin);
        int rc = collect_window_sums(ws, stream, nwin, totals.data());
        if (rc) return rc;
        *out = fold(totals.data(), c, nwin);
        return GMSM_OK;
    }
};

}  // namespace gmsm
