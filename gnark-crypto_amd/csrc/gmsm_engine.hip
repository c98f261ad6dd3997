// libgmsm.so -- C ABI (include/gmsm.h), per-device contexts and dispatch to the per-group pipelines (gmsm_group.h).
// There is no CPU fallback: every compute entry needs a usable gfx950 device and fails loudly otherwise.
#include <atomic>
#include <cstdio>
#include <cstring>
#include <deque>
#include <functional>
#include <map>
#include <sys/stat.h>

#include "gmsm_context.h"

namespace gmsm {

// Error text: per thread (like errno), plus the most recent one of the process - a cgo caller's goroutine may be moved to
// another OS thread between the failing call and gmsm_last_error().
static thread_local std::string g_last_error;
static std::mutex g_any_error_mu;
static std::string g_any_error;
// Device selection: gmsm_set_device sets the calling thread's device AND the process-wide default that threads which
// never called it inherit (a goroutine that selected a device and was then moved to a fresh OS thread still gets it).
// Entries that receive device pointers use the device that owns the pointer instead.
static thread_local int g_device = -1;
static std::atomic<int> g_default_device{0};
std::atomic<unsigned long> g_table_runs{0};
std::atomic<unsigned long> g_small_runs{0};
std::atomic<unsigned long> g_plane_runs{0};
static std::atomic<uint32_t> g_ticket_gen{0};  // ticket generations: process-wide and monotonic, so a ticket of before a gmsm_shutdown never matches one issued after it

// Process-wide switches; GMSM_C and GMSM_TABLES are read here ONCE (first use), never on a call path.
std::string g_env_error;  // a malformed GMSM_C / GMSM_TABLES: reported by the next drop-in entry (shard_devices), not dropped
Options &options() {
    static Options *o = [] {
        Options *x = new Options();
        const unsigned c = env_uint("GMSM_C", 0);
        x->window_bits.store(c >= 2 && c <= 20 ? c : 0);
        const unsigned t = env_uint("GMSM_TABLES", 1);
        x->tables.store(std::min(2u, t));
        // an out-of-range initial value is not dropped silently: the next MultiExp entry reports it (g_env_error)
        if (c != 0 && (c < 2 || c > 20)) g_env_error = "GMSM_C=" + std::to_string(c) + ": the window width must be 2..20 (or unset)";
        else if (t > 2) g_env_error = "GMSM_TABLES=" + std::to_string(t) + ": 0 never, 1 the measured call sizes, 2 every call size";
        return x;
    }();
    return *o;
}

int fail(int code, const std::string &msg) {
    g_last_error = msg;
    {
        std::lock_guard<std::mutex> lk(g_any_error_mu);
        g_any_error = msg;
    }
    return code;
}

void clear_last_error() { g_last_error.clear(); }

static std::mutex g_prof_mu;
static std::atomic<int> g_profiling{0};
static double g_stage_ms[STAGE_COUNT] = {0};
static unsigned long g_stage_launches[STAGE_COUNT] = {0};
static unsigned long g_stage_calls = 0;

int profiling_level() { return g_profiling.load(std::memory_order_relaxed); }
void record_stage_times(const float *ms, const unsigned *launches) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    for (int i = 0; i < STAGE_COUNT; ++i) {
        g_stage_ms[i] += ms[i];
        g_stage_launches[i] += launches[i];
    }
    ++g_stage_calls;
}

static std::mutex g_ctx_mu;
static std::vector<Context *> g_ctx;

int get_context_for(int device, Context **out) {
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(GMSM_ERR_DEVICE, std::string("no usable HIP device (hipGetDeviceCount: ") + hipGetErrorString(e) +
                                         "); libgmsm has no CPU fallback");
    if (device < 0 || device >= ndev) return fail(GMSM_ERR_DEVICE, "gmsm_set_device: device index out of range");
    if ((int)g_ctx.size() < ndev) g_ctx.resize(ndev, nullptr);
    if (!g_ctx[device]) g_ctx[device] = new Context();  // never deleted: gmsm_shutdown retires it (Context::retire)
    if (!g_ctx[device]->live) {  // first use, or first use after a gmsm_shutdown
        int rc = g_ctx[device]->init(device);
        if (rc != GMSM_OK) return rc;
    }
    *out = g_ctx[device];
    return GMSM_OK;
}

int get_context(Context **out) { return get_context_for(g_device >= 0 ? g_device : g_default_device.load(), out); }

int get_context_of_pointer(const void *p, Context **out) {
    if (p) {
        hipPointerAttribute_t attr;
        if (hipPointerGetAttributes(&attr, p) == hipSuccess && attr.type == hipMemoryTypeDevice)
            return get_context_for(attr.device, out);
        (void)hipGetLastError();  // not a pointer the runtime knows: fall back to the thread's device
    }
    return get_context(out);
}

// How an entry starts: the context of the calling thread's device, of a given device (the bases or the domain decide it),
// or of the device that owns a pointer - with that device made the calling thread's current one.
static int select_device(int rc, Context *const *ctx) {
    if (rc) return rc;
    HIP_TRY(hipSetDevice((*ctx)->device));
    return GMSM_OK;
}
static int enter(Context **ctx) { return select_device(get_context(ctx), ctx); }
static int enter_on(int device, Context **ctx) { return select_device(get_context_for(device, ctx), ctx); }
static int enter_owner(const void *p, Context **ctx) { return select_device(get_context_of_pointer(p, ctx), ctx); }

// Handles are index + 1 into a table that only grows: a slot that was released, or emptied by gmsm_shutdown, stays (null),
// so an old handle stays unknown and never comes to name a later registration. A reference handed out keeps the object
// alive for the caller's whole call (or ticket) even if another thread releases the handle meanwhile.
template <class T>
struct HandleTable {
    std::mutex mu;
    std::vector<std::shared_ptr<T>> slots;
    uint64_t add(std::shared_ptr<T> p) {
        std::lock_guard<std::mutex> lk(mu);
        slots.push_back(std::move(p));
        return slots.size();
    }
    std::shared_ptr<T> get(uint64_t handle) {
        std::lock_guard<std::mutex> lk(mu);
        return handle == 0 || handle > slots.size() ? nullptr : slots[handle - 1];
    }
    std::shared_ptr<T> take(uint64_t handle) {  // the table's reference: null when the handle names nothing (any more)
        std::shared_ptr<T> p;
        std::lock_guard<std::mutex> lk(mu);
        if (handle != 0 && handle <= slots.size()) p.swap(slots[handle - 1]);
        return p;
    }
    std::vector<std::shared_ptr<T>> drain() {  // every reference, the length kept
        std::vector<std::shared_ptr<T>> all;
        std::lock_guard<std::mutex> lk(mu);
        all.resize(slots.size());
        all.swap(slots);
        return all;
    }
};

// fn(i) -> return code for every i < count, each on a thread of its own; the first index that failed, with its code and
// its thread's error text (rc == GMSM_OK: none did). An index whose thread cannot be started fails with GMSM_ERR_DEVICE:
// nothing is thrown past the threads already running, or past the C ABI.
struct Failure {
    size_t index = 0;
    int rc = GMSM_OK;
    std::string err;
};
template <class F>
static Failure on_threads(size_t count, F fn) {
    std::vector<Failure> res(count);
    std::vector<std::thread> th;
    th.reserve(count);
    for (size_t i = 0; i < count; ++i) {
        res[i].index = i;
        try {
            th.emplace_back([&res, &fn, i] {
                if ((res[i].rc = fn(i))) res[i].err = gmsm_last_error();
            });
        } catch (const std::exception &e) {
            res[i].rc = GMSM_ERR_DEVICE;
            res[i].err = std::string("cannot start the worker: ") + e.what();
        }
    }
    for (auto &t : th) t.join();
    for (Failure &r : res)
        if (r.rc) return r;
    return Failure();
}

const GroupVTable *gmsm_vtable_bn254_g1();
const GroupVTable *gmsm_vtable_bn254_g2();
const GroupVTable *gmsm_vtable_bls12_381_g1();
const GroupVTable *gmsm_vtable_bls12_381_g2();
const GroupVTable *gmsm_vtable_bw6_761_g1();
const GroupVTable *gmsm_vtable_bw6_761_g2();

static const GroupVTable *vtable(int group) {
    switch (group) {
        case GMSM_BN254_G1: return gmsm_vtable_bn254_g1();
        case GMSM_BN254_G2: return gmsm_vtable_bn254_g2();
        case GMSM_BLS12_381_G1: return gmsm_vtable_bls12_381_g1();
        case GMSM_BLS12_381_G2: return gmsm_vtable_bls12_381_g2();
        case GMSM_BW6_761_G1: return gmsm_vtable_bw6_761_g1();
        case GMSM_BW6_761_G2: return gmsm_vtable_bw6_761_g2();
        default: return nullptr;
    }
}

// the scalar field's entries: one table per curve, the same for both of its groups (gmsm_field_vtable.h)
const FieldVTable *gmsm_field_vtable_bn254();
const FieldVTable *gmsm_field_vtable_bls12_381();
const FieldVTable *gmsm_field_vtable_bw6_761();

static const FieldVTable *fr_vtable(int group) {
    switch (group >> 1) {  // (a negative id stays negative or turns huge: no curve either way)
        case GMSM_BN254_G1 >> 1: return gmsm_field_vtable_bn254();
        case GMSM_BLS12_381_G1 >> 1: return gmsm_field_vtable_bls12_381();
        case GMSM_BW6_761_G1 >> 1: return gmsm_field_vtable_bw6_761();
        default: return nullptr;
    }
}

}  // namespace gmsm

using namespace gmsm;

#define GMSM_EXPORT __attribute__((visibility("default")))
#define TABLE_OR_FAIL(Table, lookup, group)        \
    const Table *vt = lookup(group);               \
    if (!vt) return fail(GMSM_ERR_ARG, "unknown group id")
#define VT_OR_FAIL(group) TABLE_OR_FAIL(GroupVTable, vtable, group)
#define FR_OR_FAIL(group) TABLE_OR_FAIL(FieldVTable, fr_vtable, group)  // an entry over the scalar field alone

// ------------------------------------------------------------------ one MultiExp over several devices
// The reference spreads one MultiExp over the cores of a machine: _innerMsmG1 starts a worker per c-bit window and
// collects one g1JacExtended per window on a channel (ecc/bn254/multiexp.go:148-209), and above a size threshold the call
// is first split in two halves of the points whose results are added (multiexp.go:98-140, AddAssign). Here the workers are
// the GPUs of the node and the split happens inside the library, below the C ABI, so that a Go caller of
// gmsm_<curve>_g1_multiexp gets all of them without knowing: one host thread per logical rank (a persistent pool, two
// workers per device like the two workspaces), each running its piece on its device through Group::shard_piece;
//   points   rank r owns points [r n/G, (r+1) n/G) and computes every window of its slice; window w of the whole MultiExp is
//            the sum of the ranks' totals for w. Each device pulls only its slice over its own PCIe link; default.
//   windows  rank r owns windows r, r+G, ... over all points (the reference's per-window workers); every device needs
//            all bases, so this only pays with bases registered on every device and few points.
// The exchange is the ranks' window totals - at most 64 extended-Jacobian points per rank, a few KB - copied from each
// device's pinned result buffer by its own host thread; an RCCL all-gather would move the same bytes device-to-device
// first and then still have to cross to the host for the fold, so the single-process form has no collective. (The
// one-process-per-GPU form of the same decomposition, with one RCCL all-gather over xGMI, is gnark-crypto_amd/sharding.py.)
// Then ONE fold (msmReduceChunk, multiexp.go:302-315) on the calling thread.
namespace gmsm {

struct ShardPool {
    struct Dev {
        std::mutex mu;
        std::condition_variable cv;
        std::deque<std::function<void()>> q;
        int workers = 0;
    };
    std::mutex mu;
    std::map<int, Dev *> devs;  // never freed: the workers outlive every static destructor
    void post(int device, std::function<void()> fn) {
        Dev *d;
        {
            std::lock_guard<std::mutex> lk(mu);
            Dev *&slot = devs[device];
            if (!slot) slot = new Dev();
            d = slot;
        }
        {
            std::lock_guard<std::mutex> lk(d->mu);
            // two workers per device; a thread that cannot be created (std::system_error) leaves through the caller's
            // handler with nothing queued - and nothing is ever queued for a device that has no worker at all
            for (; d->workers < 2; ++d->workers) {
                try {
                    std::thread([d] {
                        for (;;) {
                            std::function<void()> job;
                            {
                                std::unique_lock<std::mutex> lk2(d->mu);
                                d->cv.wait(lk2, [d] { return !d->q.empty(); });
                                job = std::move(d->q.front());
                                d->q.pop_front();
                            }
                            job();
                        }
                    }).detach();
                } catch (...) {
                    if (d->workers == 0) throw;
                    break;  // one worker serves the device
                }
            }
            d->q.push_back(std::move(fn));
        }
        d->cv.notify_one();
    }
};
static ShardPool &shard_pool() {
    static ShardPool *p = new ShardPool();
    return *p;
}

// Devices the drop-in entries spread a MultiExp over, one entry per logical rank (a device may appear more than once).
// OPT-IN (round 4; the advisor's finding): a process that configured nothing runs every drop-in call on ONE device - the
// calling thread's (gmsm_set_device) or device 0 - and creates no context, stream or worker thread anywhere else: the
// usual deployment is one prover process per GPU, and a library that silently took all eight would compete with its
// neighbours. Spreading is asked for with gmsm_set_devices(list) or GMSM_DEVICES ("0,1,2,3", or "all"), read once.
// Resolution: gmsm_set_devices; else a gmsm_set_device call pins the process to that one device; else GMSM_DEVICES;
// else no spreading. The explicit entries (gmsm_multiexp_sharded, gmsm_bases_register_sharded) with devices = NULL use the
// configured list or, when there is none, every visible device - their caller asked for several devices by name.
static std::mutex g_devices_mu;
static std::vector<int> g_devices;
static bool g_devices_explicit = false;
static std::atomic<bool> g_pinned{false};  // gmsm_set_device was called

// GMSM_DEVICES, parsed once. A malformed or out-of-range entry is an error the next drop-in call reports (it does not
// silently shrink the list): err is non-empty then.
struct EnvDevices {
    std::vector<int> list;
    std::string err;
};
static void every_device(int ndev, std::vector<int> &out) {
    for (int d = 0; d < ndev; ++d) out.push_back(d);
}
// every listed device exists; `what` is the entry (or "sharded MultiExp") the text starts with
static int devices_exist(const char *what, const int *devs, size_t count, int ndev) {
    for (size_t i = 0; i < count; ++i)
        if (devs[i] < 0 || devs[i] >= ndev)
            return fail(GMSM_ERR_DEVICE, std::string(what) + ": device " + std::to_string(devs[i]) + " does not exist (" +
                                             std::to_string(ndev) + " visible)");
    return GMSM_OK;
}
static const EnvDevices &env_devices() {
    static const EnvDevices *e = [] {
        EnvDevices *x = new EnvDevices();
        const char *v = getenv("GMSM_DEVICES");
        if (!v || !*v) return x;
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
            x->err = std::string("GMSM_DEVICES=\"") + v + "\": the device count could not be obtained (hipGetDeviceCount failed)";
            return x;
        }
        if (strcmp(v, "all") == 0) {
            every_device(ndev, x->list);
            return x;
        }
        for (const char *p = v; *p;) {
            char *end = nullptr;
            const long d = strtol(p, &end, 10);
            if (end == p || (*end && *end != ',') || (*end == ',' && !end[1])) {
                x->err = std::string("GMSM_DEVICES=\"") + v + "\": expected a comma-separated list of device indices or \"all\"";
                break;
            }
            if (d < 0 || d >= ndev) {
                x->err = std::string("GMSM_DEVICES=\"") + v + "\": device " + std::to_string(d) + " does not exist (" +
                         std::to_string(ndev) + " visible)";
                break;
            }
            x->list.push_back((int)d);
            p = *end ? end + 1 : end;
        }
        if (!x->err.empty()) x->list.clear();
        return x;
    }();
    return *e;
}

// The configured list; empty = nothing configured (or pinned). rc != 0: GMSM_DEVICES is malformed.
static int shard_devices(std::vector<int> &out) {
    out.clear();
    {
        std::lock_guard<std::mutex> lk(g_devices_mu);
        if (g_devices_explicit) {
            out = g_devices;
            return GMSM_OK;
        }
    }
    (void)options();
    if (!g_env_error.empty()) return fail(GMSM_ERR_ARG, g_env_error);
    if (g_pinned.load()) return GMSM_OK;
    const EnvDevices &e = env_devices();
    if (!e.err.empty()) return fail(GMSM_ERR_ARG, e.err);
    out = e.list;
    return GMSM_OK;
}

constexpr size_t SHARD_MIN_SLICE = (size_t)1 << 16;  // fewer points per rank than this are not worth a second device

// mode: 0 auto, 1 points, 2 windows. `replicas[d]` = bases registered on device d (full copies), or empty with `points`.
static int multiexp_sharded_run(int group, const uint64_t *points, const std::map<int, std::shared_ptr<ResidentBases>> *replicas,
                                const uint64_t *scalars, size_t n, const std::vector<int> &devs, int mode, uint64_t *out_jac) {
    const GroupVTable *vt = vtable(group);
    size_t G = devs.size();
    if (G == 0) return fail(GMSM_ERR_ARG, "sharded MultiExp: empty device list");
    if (mode == 0) mode = 1;
    if (mode != 1 && mode != 2) return fail(GMSM_ERR_ARG, "sharded MultiExp: mode must be 0 (auto), 1 (points) or 2 (windows)");
    unsigned c;
    uint32_t nwin;
    if (mode == 1) {
        G = std::max<size_t>(1, std::min(G, n / SHARD_MIN_SLICE));
        const size_t slice = (n + G - 1) / G;  // the largest slice decides c: the ranks' totals must line up
        c = choose_c(vt->fr_bits, vt->aff_bytes, slice);
        if (replicas && !replicas->empty()) {  // window tables on the replicas (gmsm_bases_precompute): their width
            const ResidentBases *rb0 = replicas->begin()->second.get();
            const unsigned forced = options().window_bits.load();
            bool all = rb0->tab_c.load() != 0;
            for (const auto &kv : *replicas) all = all && kv.second->tab_c.load() == rb0->tab_c.load();
            if (all && !(forced >= 2 && forced <= 20 && forced != rb0->tab_c.load()) && options().tables.load() != 0 &&
                vt->tables_serve(rb0->n, n / G) && vt->tables_serve(rb0->n, slice))
                c = rb0->tab_c.load();
        }
        nwin = num_windows(vt->fr_bits, c);
    } else {
        c = choose_c(vt->fr_bits, vt->aff_bytes, n);
        nwin = num_windows(vt->fr_bits, c);
        G = std::min<size_t>(G, nwin);
    }
    const size_t xl = vt->xyzz_bytes / 8;
    const uint32_t rows = mode == 1 ? nwin : (uint32_t)((nwin + G - 1) / G);
    std::vector<uint64_t> sets(G * rows * xl, 0);
    struct Result {
        int rc = GMSM_OK;
        std::string err;
    };
    std::vector<Result> res(G);
    std::mutex done_mu;
    std::condition_variable done_cv;
    size_t done = 0;
    auto piece_body = [&](size_t r) {
        Result &out = res[r];
        const int dev = devs[r];
        Context *ctx = nullptr;
        out.rc = get_context_for(dev, &ctx);
        if (out.rc == GMSM_OK && hipSetDevice(dev) != hipSuccess) out.rc = fail(GMSM_ERR_DEVICE, "hipSetDevice failed");
        if (out.rc == GMSM_OK) {  // the piece must run where its context lives: say so loudly instead of computing on a neighbour
            int cur = -1;
            if (hipGetDevice(&cur) != hipSuccess || cur != dev || ctx->device != dev)
                out.rc = fail(GMSM_ERR_DEVICE, "sharded MultiExp: rank " + std::to_string(r) + " expected device " + std::to_string(dev) +
                                                   ", the worker thread is on device " + std::to_string(cur) + " (context of device " +
                                                   std::to_string(ctx->device) + ")");
        }
        if (out.rc == GMSM_OK) {
            const ResidentBases *rb = nullptr;
            if (replicas) {
                auto it = replicas->find(dev);
                rb = it == replicas->end() ? nullptr : it->second.get();
                if (!rb) out.rc = fail(GMSM_ERR_ARG, "sharded MultiExp: the bases are not registered on device " + std::to_string(dev));
            }
            if (out.rc == GMSM_OK) {
                const size_t lo = mode == 1 ? r * n / G : 0, hi = mode == 1 ? (r + 1) * n / G : n;
                out.rc = vt->shard_piece(*ctx, points ? points + lo * (vt->aff_bytes / 8) : nullptr, rb, lo,
                                         scalars + lo * (vt->scalar_bytes / 8), hi - lo, c, mode == 1 ? 0u : (unsigned)r,
                                         mode == 1 ? 1u : (unsigned)G, sets.data() + r * rows * xl);
            }
        }
        if (out.rc != GMSM_OK) out.err = gmsm_last_error();
    };
    // Nothing may leave a piece but a return code: the workers write into this frame (sets, res) and a C caller is above us.
    auto piece = [&](size_t r) noexcept {
        try {
            piece_body(r);
        } catch (const std::exception &e) {
            res[r].rc = GMSM_ERR_DEVICE;
            res[r].err = std::string("exception in a shard piece: ") + e.what();
        } catch (...) {
            res[r].rc = GMSM_ERR_DEVICE;
            res[r].err = "unknown exception in a shard piece";
        }
    };
    size_t posted = 0;
    struct WaitAll {  // the frame outlives every worker that was handed a reference to it, whatever happens below
        std::mutex &mu;
        std::condition_variable &cv;
        size_t &done;
        const size_t &posted;
        ~WaitAll() {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return done == posted; });
        }
    };
    int prev_dev = 0;
    (void)hipGetDevice(&prev_dev);
    {
        WaitAll wait_all{done_mu, done_cv, done, posted};
        try {
            for (size_t r = 1; r < G; ++r) {
                shard_pool().post(devs[r], [&, r] {
                    piece(r);
                    std::lock_guard<std::mutex> lk(done_mu);  // the notify stays under the lock: the waiter owns these objects
                    ++done;
                    done_cv.notify_one();
                });
                ++posted;
            }
        } catch (const std::exception &e) {  // std::bad_alloc / std::system_error out of the pool: the ranks not posted fail
            for (size_t r = posted + 1; r < G; ++r) {
                res[r].rc = GMSM_ERR_DEVICE;
                res[r].err = std::string("cannot start the worker: ") + e.what();
            }
        }
        piece(0);
    }
    (void)hipSetDevice(prev_dev);
    for (size_t r = 0; r < G; ++r)
        if (res[r].rc != GMSM_OK) return fail(res[r].rc, "rank " + std::to_string(r) + " (device " + std::to_string(devs[r]) + "): " + res[r].err);
    if (mode == 1) {
        vt->fold_sets(sets.data(), (unsigned)G, c, out_jac);
    } else {
        std::vector<uint64_t> totals((size_t)nwin * xl);
        for (uint32_t w = 0; w < nwin; ++w)
            memcpy(totals.data() + (size_t)w * xl, sets.data() + ((w % G) * rows + w / G) * xl, vt->xyzz_bytes);
        vt->fold(totals.data(), c, out_jac);
    }
    return GMSM_OK;
}

// argument checks of (*G1Jac).MultiExp (multiexp.go:61-71) + the empty input, shared by the sharded entries
static int multiexp_precheck(const GroupVTable *vt, size_t n_points, size_t n_scalars, int nb_tasks, uint64_t *out_jac, bool *done) {
    *done = true;
    if (n_points != n_scalars) return fail(GMSM_ERR_LEN, "len(points) != len(scalars)");
    if (nb_tasks > 1024) return fail(GMSM_ERR_CONFIG, "invalid config: config.NbTasks > 1024");
    if (n_points == 0) return vt->multiexp_host(nullptr, 0, nullptr, 0, nb_tasks, out_jac);  // infinity (Z = 0); still needs a device
    *done = false;
    return GMSM_OK;
}

}  // namespace gmsm

extern "C" {

GMSM_EXPORT int gmsm_multiexp_sharded(int group, const uint64_t *points, size_t n_points, const uint64_t *scalars,
                                      size_t n_scalars, int nb_tasks, const int *devices, int n_devices, int mode,
                                      uint64_t *out_jac) {
    VT_OR_FAIL(group);
    bool done;
    int rc = multiexp_precheck(vt, n_points, n_scalars, nb_tasks, out_jac, &done);
    if (rc || done) return rc;
    std::vector<int> devs;
    if (devices && n_devices > 0) devs.assign(devices, devices + n_devices);
    else if ((rc = shard_devices(devs))) return rc;
    if (devs.empty()) {  // nothing configured: the caller asked for a sharded call, so every visible device
        int ndev = gmsm_device_count();
        if (ndev <= 0) return fail(GMSM_ERR_DEVICE, "no usable HIP device; libgmsm has no CPU fallback");
        every_device(ndev, devs);
    }
    if ((rc = devices_exist("sharded MultiExp", devs.data(), devs.size(), gmsm_device_count()))) return rc;
    return multiexp_sharded_run(group, points, nullptr, scalars, n_points, devs, mode, out_jac);
}

GMSM_EXPORT int gmsm_multiexp(int group, const uint64_t *points, size_t n_points, const uint64_t *scalars,
                              size_t n_scalars, int nb_tasks, uint64_t *out_jac) {
    VT_OR_FAIL(group);
    // more than one device CONFIGURED (gmsm_set_devices / GMSM_DEVICES - spreading is opt-in) and enough points for two
    // slices: the call is spread over them
    if (n_points == n_scalars && nb_tasks <= 1024 && n_points >= 2 * SHARD_MIN_SLICE) {
        std::vector<int> devs;
        int rc = shard_devices(devs);
        if (rc) return rc;
        if (devs.size() > 1) return multiexp_sharded_run(group, points, nullptr, scalars, n_points, devs, 0, out_jac);
    }
    return vt->multiexp_host(points, n_points, scalars, n_scalars, nb_tasks, out_jac);
}

#define GMSM_DROPIN(name, id)                                                                                \
    GMSM_EXPORT int gmsm_##name##_multiexp(const uint64_t *points, size_t n_points, const uint64_t *scalars, \
                                           size_t n_scalars, int nb_tasks, uint64_t *out_jac) {              \
        return gmsm_multiexp(id, points, n_points, scalars, n_scalars, nb_tasks, out_jac);                   \
    }
GMSM_DROPIN(bn254_g1, GMSM_BN254_G1)
GMSM_DROPIN(bn254_g2, GMSM_BN254_G2)
GMSM_DROPIN(bls12_381_g1, GMSM_BLS12_381_G1)
GMSM_DROPIN(bls12_381_g2, GMSM_BLS12_381_G2)
GMSM_DROPIN(bw6_761_g1, GMSM_BW6_761_G1)
GMSM_DROPIN(bw6_761_g2, GMSM_BW6_761_G2)

GMSM_EXPORT int gmsm_multiexp_affine(int group, const uint64_t *points, size_t n_points, const uint64_t *scalars,
                                     size_t n_scalars, int nb_tasks, uint64_t *out_affine) {
    VT_OR_FAIL(group);
    std::vector<uint64_t> jac(vt->jac_bytes / 8);
    int rc = gmsm_multiexp(group, points, n_points, scalars, n_scalars, nb_tasks, jac.data());
    if (rc) return rc;
    vt->jac_to_affine(jac.data(), out_affine);
    return GMSM_OK;
}

GMSM_EXPORT int gmsm_fold(int group, const uint64_t *points, size_t n_points, const uint64_t *combination_coeff,
                          int nb_tasks, uint64_t *out_jac) {
    VT_OR_FAIL(group);
    if (!combination_coeff) return fail(GMSM_ERR_ARG, "combination_coeff is null");
    if (!out_jac || (n_points && !points)) return fail(GMSM_ERR_ARG, "gmsm_fold: null argument");
    if (nb_tasks > 1024) return fail(GMSM_ERR_CONFIG, "invalid config: config.NbTasks > 1024");
    if (n_points >= ((size_t)1 << 31)) return fail(GMSM_ERR_ARG, "n must be < 2^31");
    std::vector<uint64_t> powers;  // 1, g, g^2, ... (multiexp.go:331-337)
    try {
        powers.resize(n_points * (vt->scalar_bytes / 8));
    } catch (const std::exception &) {
        return fail(GMSM_ERR_DEVICE, "gmsm_fold: out of host memory for the powers of the coefficient");
    }
    vt->fold_powers(combination_coeff, n_points, powers.data());
    return gmsm_multiexp(group, points, n_points, powers.data(), n_points, nb_tasks, out_jac);
}

GMSM_EXPORT int gmsm_multiexp_device(int group, const void *d_points, const void *d_scalars, size_t n, void *hip_stream,
                                     uint64_t *out_jac) {
    VT_OR_FAIL(group);
    Context *ctx;
    if (int rc = enter_owner(d_scalars ? d_scalars : d_points, &ctx)) return rc;
    return vt->multiexp_device(*ctx, d_points, d_scalars, n, (hipStream_t)hip_stream, out_jac, nullptr);
}

// ------------------------------------------------------------------ resident bases
using BasesRef = std::shared_ptr<ResidentBases>;
// g_bases and g_sharded (below) each have their lock: no entry looks at both tables under one lock - gmsm_bases_release takes
// from the one its handle's tag names - and gmsm_shutdown, which empties both, runs alone by its contract.
static HandleTable<ResidentBases> g_bases;

// new bases of `group` on the call's device from n affine points in device memory, and their handle
static int register_device_points(const GroupVTable *vt, Context *ctx, Workspace &ws, int group, const void *d_points,
                                  size_t n, uint64_t *out_handle) {
    BasesRef rb = std::make_shared<ResidentBases>();
    rb->group = group;
    rb->device = ctx->device;
    int rc = vt->register_bases(*ctx, d_points, n, ws.stream, rb.get());
    if (rc) return rc;  // ~ResidentBases frees whatever was allocated
    *out_handle = g_bases.add(rb);
    return GMSM_OK;
}

GMSM_EXPORT int gmsm_bases_register(int group, const uint64_t *points, const void *d_points, size_t n,
                                    uint64_t *out_handle) {
    VT_OR_FAIL(group);
    if (!out_handle) return fail(GMSM_ERR_ARG, "gmsm_bases_register: out_handle is null");
    if ((points == nullptr) == (d_points == nullptr) && n)
        return fail(GMSM_ERR_ARG, "gmsm_bases_register: give exactly one of points (host) / d_points (device)");
    Context *ctx;
    int rc = enter_owner(d_points, &ctx);
    if (rc) return rc;
    GMSM_LEASE_OR_FAIL(lease, *ctx);
    Workspace &ws = *lease.w;
    const void *src;
    if ((rc = stage_input(ws, ws.h2d_points, points, d_points, n * vt->aff_bytes, {After::DEVICE}, &src))) return rc;
    return register_device_points(vt, ctx, ws, group, src, n, out_handle);
}

// ------------------------------------------------------------------ point ingest
// what a decode or a validation found: GMSM_OK, or the first offender's position in *bad_index and its status as the text
static int point_result(const char *what, long long bad, uint32_t status, int64_t *bad_index) {
    if (bad < 0) return GMSM_OK;
    *bad_index = bad;
    return fail(GMSM_ERR_POINT, std::string(what) + ": point " + std::to_string(bad) + ": " + point_status_text(status));
}

// The two wire formats of the ingest entries: RawBytes() output (X and Y), and the Encoder's default, compressed, format: X
// and the flag of Y's half (gmsm_decompress.h), half the bytes.
struct WireFormat {
    const char *arg;  // the entries' name for the encoded bytes
    size_t shrink;    // encoded bytes of a point = aff_bytes / shrink
    decltype(GroupVTable::decode_raw) GroupVTable::*decode;
};
static const WireFormat WIRE_RAW = {"raw", 1, &GroupVTable::decode_raw}, WIRE_COMPRESSED = {"comp", 2, &GroupVTable::decode_compressed};

static int points_decode(const char *E, const WireFormat &wire, int group, const uint8_t *enc, size_t n, int check, uint64_t *out_affine,
                         void *d_out_affine, int64_t *bad_index) {
    VT_OR_FAIL(group);
    if (!bad_index) return fail(GMSM_ERR_ARG, std::string(E) + ": bad_index is null");
    *bad_index = -1;
    if (n && (!enc || (!out_affine && !d_out_affine))) return fail(GMSM_ERR_ARG, std::string(E) + ": null argument");
    if (n == 0) return GMSM_OK;
    Context *ctx;
    int rc = enter_owner(d_out_affine, &ctx);
    if (rc) return rc;
    GMSM_LEASE_OR_FAIL(lease, *ctx);
    Workspace &ws = *lease.w;
    const size_t bytes = n * vt->aff_bytes, ebytes = bytes / wire.shrink;
    if ((rc = ws.raw_bytes.ensure(ebytes))) return rc;
    void *d_out = d_out_affine;
    if (!d_out) {
        if ((rc = ws.h2d_points.ensure(bytes))) return rc;
        d_out = ws.h2d_points.ptr;
    }
    HIP_TRY(hipMemcpyAsync(ws.raw_bytes.ptr, enc, ebytes, hipMemcpyHostToDevice, ws.stream));
    long long bad = -1;
    uint32_t status = 0;
    if ((rc = (vt->*wire.decode)(ws, ws.raw_bytes.ptr, n, check, d_out, &bad, &status))) return rc;
    if (out_affine) {
        HIP_TRY(hipMemcpyAsync(out_affine, d_out, bytes, hipMemcpyDeviceToHost, ws.stream));
        HIP_TRY(hipStreamSynchronize(ws.stream));
    }
    return point_result(E, bad, status, bad_index);
}

static int bases_register_encoded(const char *E, const WireFormat &wire, int group, const uint8_t *enc, size_t n, int check,
                                  uint64_t *out_handle, int64_t *bad_index) {
    VT_OR_FAIL(group);
    if (!out_handle || !bad_index) return fail(GMSM_ERR_ARG, std::string(E) + ": null argument");
    *bad_index = -1;
    if (n && !enc) return fail(GMSM_ERR_ARG, std::string(E) + ": " + wire.arg + " is null");
    Context *ctx;
    int rc = enter(&ctx);
    if (rc) return rc;
    GMSM_LEASE_OR_FAIL(lease, *ctx);
    Workspace &ws = *lease.w;
    const size_t bytes = n * vt->aff_bytes, ebytes = bytes / wire.shrink;
    if (n) {
        if ((rc = ws.raw_bytes.ensure(ebytes))) return rc;
        if ((rc = ws.h2d_points.ensure(bytes))) return rc;
        HIP_TRY(hipMemcpyAsync(ws.raw_bytes.ptr, enc, ebytes, hipMemcpyHostToDevice, ws.stream));
        long long bad = -1;
        uint32_t status = 0;
        if ((rc = (vt->*wire.decode)(ws, ws.raw_bytes.ptr, n, check, ws.h2d_points.ptr, &bad, &status))) return rc;
        if ((rc = point_result(E, bad, status, bad_index))) return rc;
    }
    return register_device_points(vt, ctx, ws, group, ws.h2d_points.ptr, n, out_handle);
}

GMSM_EXPORT int gmsm_points_from_raw(int group, const uint8_t *raw, size_t n, int check, uint64_t *out_affine,
                                     void *d_out_affine, int64_t *bad_index) {
    return points_decode("gmsm_points_from_raw", WIRE_RAW, group, raw, n, check, out_affine, d_out_affine, bad_index);
}

GMSM_EXPORT int gmsm_points_validate(int group, const uint64_t *points, const void *d_points, size_t n, int check,
                                     int64_t *bad_index) {
    VT_OR_FAIL(group);
    if (!bad_index) return fail(GMSM_ERR_ARG, "gmsm_points_validate: bad_index is null");
    *bad_index = -1;
    if (n && (points == nullptr) == (d_points == nullptr))
        return fail(GMSM_ERR_ARG, "gmsm_points_validate: give exactly one of points (host) / d_points (device)");
    if (n == 0 || check <= 0) return GMSM_OK;
    Context *ctx;
    int rc = enter_owner(d_points, &ctx);
    if (rc) return rc;
    GMSM_LEASE_OR_FAIL(lease, *ctx);
    Workspace &ws = *lease.w;
    const void *src;
    if ((rc = stage_input(ws, ws.h2d_points, points, d_points, n * vt->aff_bytes, {After::DEVICE}, &src))) return rc;
    long long bad = -1;
    uint32_t status = 0;
    if ((rc = vt->validate_points(ws, src, n, check, &bad, &status))) return rc;
    return point_result("gmsm_points_validate", bad, status, bad_index);
}

GMSM_EXPORT int gmsm_bases_register_raw(int group, const uint8_t *raw, size_t n, int check, uint64_t *out_handle,
                                        int64_t *bad_index) {
    return bases_register_encoded("gmsm_bases_register_raw", WIRE_RAW, group, raw, n, check, out_handle, bad_index);
}

GMSM_EXPORT int gmsm_points_from_compressed(int group, const uint8_t *comp, size_t n, int check, uint64_t *out_affine,
                                            void *d_out_affine, int64_t *bad_index) {
    return points_decode("gmsm_points_from_compressed", WIRE_COMPRESSED, group, comp, n, check, out_affine, d_out_affine, bad_index);
}

GMSM_EXPORT int gmsm_points_compress(int group, const uint64_t *points, const void *d_points, size_t n, uint8_t *out_comp) {
    VT_OR_FAIL(group);
    if (n && ((points == nullptr) == (d_points == nullptr) || !out_comp))
        return fail(GMSM_ERR_ARG, "gmsm_points_compress: give exactly one of points (host) / d_points (device), and out_comp");
    if (n == 0) return GMSM_OK;
    Context *ctx;
    int rc = enter_owner(d_points, &ctx);
    if (rc) return rc;
    GMSM_LEASE_OR_FAIL(lease, *ctx);
    Workspace &ws = *lease.w;
    const size_t bytes = n * vt->aff_bytes, cbytes = bytes / 2;
    if ((rc = ws.raw_bytes.ensure(cbytes))) return rc;
    const void *src;
    if ((rc = stage_input(ws, ws.h2d_points, points, d_points, bytes, {After::DEVICE}, &src))) return rc;
    if ((rc = vt->encode_compressed(ws, src, n, ws.raw_bytes.ptr))) return rc;
    HIP_TRY(hipMemcpyAsync(out_comp, ws.raw_bytes.ptr, cbytes, hipMemcpyDeviceToHost, ws.stream));
    HIP_TRY(hipStreamSynchronize(ws.stream));
    return GMSM_OK;
}

GMSM_EXPORT int gmsm_bases_register_compressed(int group, const uint8_t *comp, size_t n, int check, uint64_t *out_handle,
                                               int64_t *bad_index) {
    return bases_register_encoded("gmsm_bases_register_compressed", WIRE_COMPRESSED, group, comp, n, check, out_handle, bad_index);
}

GMSM_EXPORT int gmsm_bases_register_dump(int group, const char *path, uint64_t offset, int expect_marker, size_t max_points,
                                         int check, uint64_t *out_handle, size_t *out_n, int64_t *bad_index) {
    VT_OR_FAIL(group);
    if (!path || !out_handle || !out_n || !bad_index) return fail(GMSM_ERR_ARG, "gmsm_bases_register_dump: null argument");
    *bad_index = -1;
    *out_n = 0;
    FILE *f = fopen(path, "rb");
    if (!f) return fail(GMSM_ERR_ARG, std::string("gmsm_bases_register_dump: cannot open ") + path);
    struct Closer {
        FILE *f;
        ~Closer() { fclose(f); }
    } closer{f};
    if (fseeko(f, (off_t)offset, SEEK_SET) != 0) return fail(GMSM_ERR_ARG, "gmsm_bases_register_dump: bad offset");
    uint64_t word = 0;
    if (expect_marker) {  // unsafe.ReadMarker, utils/unsafe/dump_slice.go:91-103
        if (fread(&word, 8, 1, f) != 1) return fail(GMSM_ERR_ARG, "gmsm_bases_register_dump: short read (marker)");
        if (word != 0xdeadbeefull)
            return fail(GMSM_ERR_ARG, "marker mismatch: dump was not written on the same architecture");
    }
    if (fread(&word, 8, 1, f) != 1) return fail(GMSM_ERR_ARG, "gmsm_bases_register_dump: short read (length)");
    size_t n = (size_t)word;
    if (max_points && n > max_points) n = max_points;  // ReadSlice's maxElements
    if (n >= ((size_t)1 << 31)) return fail(GMSM_ERR_ARG, "gmsm_bases_register_dump: more than 2^31 points");
    {   // the length word comes from the file: believe it only as far as the file goes (before any device memory is asked for)
        const off_t here = ftello(f);
        struct stat st;
        if (here >= 0 && fstat(fileno(f), &st) == 0 && S_ISREG(st.st_mode)) {
            const uint64_t left = st.st_size > here ? (uint64_t)(st.st_size - here) : 0;
            if ((uint64_t)n * vt->aff_bytes > left)
                return fail(GMSM_ERR_ARG, "gmsm_bases_register_dump: short read (points): the file holds fewer points than its length word says");
        }
    }
    Context *ctx;
    int rc = enter(&ctx);
    if (rc) return rc;
    GMSM_LEASE_OR_FAIL(lease, *ctx);
    Workspace &ws = *lease.w;
    const size_t bytes = n * vt->aff_bytes;
    if (n) {
        if ((rc = ws.h2d_points.ensure(bytes))) return rc;
        // file -> two pinned buffers -> HBM: the read of chunk k+1 runs while chunk k crosses PCIe
        constexpr size_t CHUNK = (size_t)32 << 20;
        void *pin[2] = {nullptr, nullptr};
        hipEvent_t done[2] = {nullptr, nullptr};
        auto cleanup = [&]() {
            for (int i = 0; i < 2; ++i) {
                if (done[i]) (void)hipEventDestroy(done[i]);
                if (pin[i]) (void)hipHostFree(pin[i]);
            }
        };
        for (int i = 0; i < 2; ++i) {
            if (hipHostMalloc(&pin[i], CHUNK, hipHostMallocDefault) != hipSuccess ||
                hipEventCreateWithFlags(&done[i], hipEventDisableTiming) != hipSuccess) {
                cleanup();
                return fail(GMSM_ERR_DEVICE, "gmsm_bases_register_dump: cannot allocate pinned staging buffers");
            }
        }
        size_t pos = 0;
        for (unsigned k = 0; pos < bytes; ++k) {
            const size_t len = std::min(CHUNK, bytes - pos);
            const int b = (int)(k & 1u);
            if (k >= 2) (void)hipEventSynchronize(done[b]);
            if (fread(pin[b], 1, len, f) != len) {
                (void)hipStreamSynchronize(ws.stream);
                cleanup();
                return fail(GMSM_ERR_ARG, "gmsm_bases_register_dump: short read (points)");
            }
            hipError_t e = hipMemcpyAsync((char *)ws.h2d_points.ptr + pos, pin[b], len, hipMemcpyHostToDevice, ws.stream);
            if (e == hipSuccess) e = hipEventRecord(done[b], ws.stream);
            if (e != hipSuccess) {
                (void)hipStreamSynchronize(ws.stream);
                cleanup();
                return fail(GMSM_ERR_DEVICE, std::string("gmsm_bases_register_dump: ") + hipGetErrorString(e));
            }
            pos += len;
        }
        (void)hipStreamSynchronize(ws.stream);
        cleanup();
        if (check > 0) {
            long long bad = -1;
            uint32_t status = 0;
            if ((rc = vt->validate_points(ws, ws.h2d_points.ptr, n, check, &bad, &status))) return rc;
            if ((rc = point_result("gmsm_bases_register_dump", bad, status, bad_index))) return rc;
        }
    }
    if ((rc = register_device_points(vt, ctx, ws, group, ws.h2d_points.ptr, n, out_handle))) return rc;
    *out_n = n;
    return GMSM_OK;
}

// Bases registered on several devices (full copies: 1 GiB per device for 2^24 BN254 G1 points, of 288 GB): any prefix of
// them can then be cut into equal point slices - or into window sets - over the ranks, whatever its length.
struct ShardedBases {
    int group = -1;
    size_t n = 0;
    std::vector<int> devices;                                  // logical ranks
    std::map<int, std::shared_ptr<ResidentBases>> replicas;    // device -> its copy
};
constexpr uint64_t SHARDED_TAG = (uint64_t)1 << 62;
static HandleTable<ShardedBases> g_sharded;  // handle = SHARDED_TAG | the table's

static std::shared_ptr<ShardedBases> lookup_sharded(uint64_t handle) {
    return (handle & SHARDED_TAG) ? g_sharded.get(handle & ~SHARDED_TAG) : nullptr;
}

GMSM_EXPORT int gmsm_bases_register_sharded(int group, const uint64_t *points, size_t n, const int *devices, int n_devices,
                                            uint64_t *out_handle) {
    VT_OR_FAIL(group);
    if (!out_handle) return fail(GMSM_ERR_ARG, "gmsm_bases_register_sharded: out_handle is null");
    if (n && !points) return fail(GMSM_ERR_ARG, "gmsm_bases_register_sharded: points is null");
    auto sb = std::make_shared<ShardedBases>();
    sb->group = group;
    sb->n = n;
    if (devices && n_devices > 0) sb->devices.assign(devices, devices + n_devices);
    else if (int rc0 = shard_devices(sb->devices)) return rc0;
    const int ndev = gmsm_device_count();
    if (ndev <= 0) return fail(GMSM_ERR_DEVICE, "no usable HIP device; libgmsm has no CPU fallback");
    if (sb->devices.empty()) every_device(ndev, sb->devices);
    if (int rc = devices_exist("gmsm_bases_register_sharded", sb->devices.data(), sb->devices.size(), ndev)) return rc;
    // one upload per distinct device, all of them at once (every device has its own PCIe link)
    std::vector<int> distinct;
    for (int d : sb->devices)
        if (std::find(distinct.begin(), distinct.end(), d) == distinct.end()) distinct.push_back(d);
    std::vector<uint64_t> handles(distinct.size(), 0);
    const Failure bad = on_threads(distinct.size(), [&](size_t i) {
        g_device = distinct[i];  // the worker's own device: gmsm_bases_register uploads to the calling thread's
        return gmsm_bases_register(group, points, nullptr, n, &handles[i]);
    });
    for (size_t i = 0; i < distinct.size(); ++i)
        if (handles[i]) {
            sb->replicas[distinct[i]] = g_bases.get(handles[i]);
            (void)gmsm_bases_release(handles[i]);  // the per-device table entry goes; `replicas` keeps the bases alive
        }
    if (bad.rc) return fail(bad.rc, "device " + std::to_string(distinct[bad.index]) + ": " + bad.err);
    *out_handle = SHARDED_TAG | g_sharded.add(sb);
    return GMSM_OK;
}

// Window tables of registered bases: slab w = 2^(c w) P_i for every window of the c-bit decomposition, nwin copies of
// the bases in HBM; MultiExp calls over the handle then fill ONE bucket set (Group::precompute_tables). c = 0: the
// library's width for this many bases.
static int precompute_on(const BasesRef &rb, unsigned c) {
    const GroupVTable *vt = vtable(rb->group);
    std::lock_guard<std::mutex> only_one(rb->tab_mu);
    if (rb->tab_c.load() != 0) {
        if (c == 0 || c == rb->tab_c.load()) return GMSM_OK;
        return fail(GMSM_ERR_ARG, "gmsm_bases_precompute: the handle already has tables of another width");
    }
    Context *ctx;
    int rc = get_context_for(rb->device, &ctx);
    if (rc) return rc;
    struct RestoreDevice {  // every exit path leaves the calling thread on the device it came with
        int prev = 0;
        RestoreDevice() { (void)hipGetDevice(&prev); }
        ~RestoreDevice() { (void)hipSetDevice(prev); }
    } restore;
    HIP_TRY(hipSetDevice(ctx->device));
    GMSM_LEASE_OR_FAIL(lease, *ctx);
    return vt->precompute_tables(*ctx, *lease.w, rb.get(), c);
}

GMSM_EXPORT int gmsm_bases_precompute(uint64_t handle, unsigned c) {
    if (handle & SHARDED_TAG) {
        std::shared_ptr<ShardedBases> sb = lookup_sharded(handle);
        if (!sb) return fail(GMSM_ERR_ARG, "unknown bases handle");
        std::vector<BasesRef> replicas;
        for (auto &kv : sb->replicas) replicas.push_back(kv.second);
        const Failure bad = on_threads(replicas.size(), [&](size_t i) { return precompute_on(replicas[i], c); });
        return bad.rc ? fail(bad.rc, bad.err) : GMSM_OK;
    }
    BasesRef rb = g_bases.get(handle);
    if (!rb) return fail(GMSM_ERR_ARG, "unknown bases handle");
    return precompute_on(rb, c);
}

GMSM_EXPORT unsigned long gmsm_debug_table_runs(void) { return g_table_runs.load(); }
GMSM_EXPORT unsigned long gmsm_debug_small_runs(void) { return g_small_runs.load(); }
GMSM_EXPORT unsigned long gmsm_debug_plane_runs(void) { return g_plane_runs.load(); }

// 0 = no tables; else the window width of the handle's tables
GMSM_EXPORT unsigned gmsm_bases_table_bits(uint64_t handle) {
    if (handle & SHARDED_TAG) {
        std::shared_ptr<ShardedBases> sb = lookup_sharded(handle);
        if (!sb || sb->replicas.empty()) return 0;
        return sb->replicas.begin()->second->tab_c.load();
    }
    BasesRef rb = g_bases.get(handle);
    return rb ? rb->tab_c.load() : 0;
}

GMSM_EXPORT int gmsm_bases_release(uint64_t handle) {
    BasesRef rb;
    std::shared_ptr<ShardedBases> sb;
    if (handle & SHARDED_TAG) sb = g_sharded.take(handle & ~SHARDED_TAG);
    else rb = g_bases.take(handle);
    if (!rb && !sb) return fail(GMSM_ERR_ARG, "unknown bases handle");
    // Calls and tickets that are still using the bases hold their own references; the memory goes with the last one. A
    // reference that an enqueue-only call parked on an idle workspace would otherwise live until that workspace is leased
    // again: drop it here once its work has finished (outside the context lock - the destructor synchronises the device).
    std::vector<Context *> ctxs;
    {
        std::lock_guard<std::mutex> lk(g_ctx_mu);
        ctxs = g_ctx;
    }
    for (Context *c : ctxs) {
        if (!c) continue;
        BasesRef parked[Context::NUM_WS];
        {
            std::lock_guard<std::mutex> lk(c->mu);
            for (int i = 0; i < Context::NUM_WS; ++i) {
                Workspace &w = c->ws[i];
                if (w.busy || !w.bases_ref) continue;
                const bool mine = w.bases_ref == rb || (sb && sb->replicas.count(c->device) && sb->replicas[c->device] == w.bases_ref);
                if (mine && (!w.last_use || hipEventQuery(w.last_use) == hipSuccess)) parked[i].swap(w.bases_ref);
            }
        }
    }
    return GMSM_OK;
}

static int multiexp_bases_impl(uint64_t handle, const uint64_t *scalars, const void *d_scalars, size_t n, int nb_tasks,
                               void *hip_stream, uint64_t *out_jac) {
    BasesRef rb = g_bases.get(handle);
    if (!rb) return fail(GMSM_ERR_ARG, "unknown bases handle");
    const GroupVTable *vt = vtable(rb->group);
    if (n > rb->n) return fail(GMSM_ERR_LEN, "len(points) != len(scalars)");  // more scalars than registered bases
    if (nb_tasks > 1024) return fail(GMSM_ERR_CONFIG, "invalid config: config.NbTasks > 1024");
    Context *ctx;
    if (int rc = enter_on(rb->device, &ctx)) return rc;  // the bases decide the device, not the calling thread
    if (scalars && n) return vt->multiexp_bases_host(*ctx, scalars, n, out_jac, rb.get());
    return vt->multiexp_device(*ctx, nullptr, d_scalars, n, (hipStream_t)hip_stream, out_jac, rb.get());
}

static int multiexp_bases_sharded(uint64_t handle, const uint64_t *scalars, size_t n, int nb_tasks, int mode, uint64_t *out_jac) {
    std::shared_ptr<ShardedBases> sb = lookup_sharded(handle);
    if (!sb) return fail(GMSM_ERR_ARG, "unknown bases handle");
    const GroupVTable *vt = vtable(sb->group);
    if (n > sb->n) return fail(GMSM_ERR_LEN, "len(points) != len(scalars)");  // more scalars than registered bases
    bool done;
    int rc = multiexp_precheck(vt, n, n, nb_tasks, out_jac, &done);
    if (rc || done) return rc;
    if (!scalars) return fail(GMSM_ERR_ARG, "scalars is null");
    return multiexp_sharded_run(sb->group, nullptr, &sb->replicas, scalars, n, sb->devices, mode, out_jac);
}

GMSM_EXPORT int gmsm_multiexp_bases(uint64_t handle, const uint64_t *scalars, size_t n_scalars, int nb_tasks,
                                    uint64_t *out_jac) {
    if (handle & SHARDED_TAG) return multiexp_bases_sharded(handle, scalars, n_scalars, nb_tasks, 0, out_jac);
    return multiexp_bases_impl(handle, scalars, nullptr, n_scalars, nb_tasks, nullptr, out_jac);
}

GMSM_EXPORT int gmsm_multiexp_bases_sharded(uint64_t handle, const uint64_t *scalars, size_t n_scalars, int nb_tasks, int mode,
                                            uint64_t *out_jac) {
    if (!(handle & SHARDED_TAG)) return fail(GMSM_ERR_ARG, "gmsm_multiexp_bases_sharded: not a handle of gmsm_bases_register_sharded");
    return multiexp_bases_sharded(handle, scalars, n_scalars, nb_tasks, mode, out_jac);
}

GMSM_EXPORT int gmsm_multiexp_bases_device(uint64_t handle, const void *d_scalars, size_t n_scalars, void *hip_stream,
                                           uint64_t *out_jac) {
    return multiexp_bases_impl(handle, nullptr, d_scalars, n_scalars, 0, hip_stream, out_jac);
}

// ------------------------------------------------------------------ two MultiExp calls in flight
// ticket = device << 40 | generation << 8 | (slot + 1)
GMSM_EXPORT int gmsm_multiexp_bases_submit(uint64_t handle, const void *d_scalars, size_t n_scalars, void *hip_stream,
                                           uint64_t *out_ticket) {
    BasesRef rb = g_bases.get(handle);
    if (!rb) return fail(GMSM_ERR_ARG, "unknown bases handle");
    if (!out_ticket) return fail(GMSM_ERR_ARG, "out_ticket is null");
    const GroupVTable *vt = vtable(rb->group);
    if (n_scalars > rb->n) return fail(GMSM_ERR_LEN, "len(points) != len(scalars)");
    Context *ctx;
    int rc = enter_on(rb->device, &ctx);
    if (rc) return rc;
    int why = 0;
    Lease lease(*ctx, /*wait=*/false, /*for_ticket=*/true, &why);
    Workspace *ws = lease.w;
    if (!ws)
        return why == 1 ? fail(GMSM_ERR_ARG, "two submitted MultiExp calls are outstanding on this device: collect one first")
                        : fail(GMSM_ERR_DEVICE, "gmsm_shutdown ran while this submit waited for a workspace");
    // the scalars are produced on the caller's stream (NULL = the default stream): order our stream behind it
    if ((rc = order_after(*ws, (hipStream_t)hip_stream))) return rc;
    if ((rc = vt->submit(*ctx, *ws, d_scalars, n_scalars, rb.get()))) return rc;
    lease.keep();  // released by gmsm_multiexp_collect
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        ws->bases_ref = rb;  // the ticket owns a reference until it is collected
        ws->pending = true;
        ws->pending_group = rb->group;
        ws->pending_gen = g_ticket_gen.fetch_add(1, std::memory_order_relaxed) + 1;  // unique across gmsm_shutdown
    }
    *out_ticket = ((uint64_t)ctx->device << 40) | ((uint64_t)(ws->pending_gen & 0xffffffffu) << 8) | (uint64_t)(ws - ctx->ws + 1);
    return GMSM_OK;
}

// k MultiExp over the same registered bases, one scalar vector each (kzg.Commit over many polynomials with one SRS,
// ecc/bn254/kzg/kzg.go:159-176, 246-300): a single blocking call that keeps two of them in flight. With host scalars
// the copy of vector i+1 runs while vector i is being accumulated.
static int multiexp_bases_batch_on(const BasesRef &rb, const uint64_t *scalars, const void *d_scalars, size_t n, size_t k,
                                   void *hip_stream, uint64_t *out_jac);

GMSM_EXPORT int gmsm_multiexp_bases_batch(uint64_t handle, const uint64_t *scalars, const void *d_scalars, size_t n,
                                          size_t k, void *hip_stream, uint64_t *out_jac) {
    if (handle & SHARDED_TAG) {
        // Bases registered on several devices: the k vectors are independent MultiExp calls, so they need no sharding of
        // a single one - rank r (one host thread per logical rank) runs the contiguous block of vectors [r k/G, (r+1) k/G)
        // on its device's copy of the bases; no exchange at all (the replica mode of sharding.py, inside the library).
        std::shared_ptr<ShardedBases> sb = lookup_sharded(handle);
        if (!sb) return fail(GMSM_ERR_ARG, "unknown bases handle");
        if (n > sb->n) return fail(GMSM_ERR_LEN, "len(points) != len(scalars)");
        if (k == 0) return GMSM_OK;
        if (n && !scalars) return fail(GMSM_ERR_ARG, "gmsm_multiexp_bases_batch: a sharded handle takes host scalars");
        const GroupVTable *vts = vtable(sb->group);
        const size_t G = std::min<size_t>(sb->devices.size(), k), jl = vts->jac_bytes / 8, sl = vts->scalar_bytes / 8 * n;
        const Failure bad = on_threads(G, [&](size_t r) {
            const size_t lo = r * k / G, hi = (r + 1) * k / G;
            const BasesRef &rb = sb->replicas.at(sb->devices[r]);
            return multiexp_bases_batch_on(rb, scalars ? scalars + lo * sl : nullptr, nullptr, n, hi - lo, nullptr, out_jac + lo * jl);
        });
        if (bad.rc) return fail(bad.rc, "rank " + std::to_string(bad.index) + " (device " + std::to_string(sb->devices[bad.index]) + "): " + bad.err);
        return GMSM_OK;
    }
    BasesRef rb = g_bases.get(handle);
    if (!rb) return fail(GMSM_ERR_ARG, "unknown bases handle");
    if (n > rb->n) return fail(GMSM_ERR_LEN, "len(points) != len(scalars)");
    if (k == 0) return GMSM_OK;
    if (n && (scalars == nullptr) == (d_scalars == nullptr))
        return fail(GMSM_ERR_ARG, "gmsm_multiexp_bases_batch: give exactly one of scalars (host) / d_scalars (device)");
    return multiexp_bases_batch_on(rb, scalars, d_scalars, n, k, hip_stream, out_jac);
}

static int multiexp_bases_batch_on(const BasesRef &rb, const uint64_t *scalars, const void *d_scalars, size_t n, size_t k,
                                   void *hip_stream, uint64_t *out_jac) {
    const GroupVTable *vt = vtable(rb->group);
    Context *ctx;
    int rc = enter_on(rb->device, &ctx);
    if (rc) return rc;
    const size_t jl = vt->jac_bytes / 8, sb = vt->scalar_bytes * n;
    if (n == 0) {
        for (size_t i = 0; i < k; ++i)
            if ((rc = vt->multiexp_device(*ctx, nullptr, nullptr, 0, nullptr, out_jac + i * jl, rb.get()))) return rc;
        return GMSM_OK;
    }
    Workspace *w[2] = {ctx->acquire(true), nullptr};
    if (!w[0]) return fail(GMSM_ERR_DEVICE, "no workspace could be leased (internal error)");
    w[1] = ctx->acquire(false);  // a concurrent caller may hold it: then this batch runs one call at a time
    const size_t nws = w[1] ? 2 : 1;
    size_t submitted = 0, collected = 0;
    rc = GMSM_OK;
    while (rc == GMSM_OK && collected < k) {
        while (rc == GMSM_OK && submitted < k && submitted - collected < nws) {
            Workspace &ws = *w[submitted % nws];
            const void *dsc;  // written out, not stage_input: a failed copy must end the loop, and has a text of its own
            if (scalars) {
                if ((rc = ws.h2d_scalars.ensure(sb))) break;
                hipError_t e = hipMemcpyAsync(ws.h2d_scalars.ptr, (const char *)scalars + submitted * sb, sb,
                                              hipMemcpyHostToDevice, ws.stream);
                if (e != hipSuccess) {
                    rc = fail(GMSM_ERR_DEVICE, std::string("hipMemcpyAsync: ") + hipGetErrorString(e));
                    break;
                }
                dsc = ws.h2d_scalars.ptr;
            } else {
                if ((rc = order_after(ws, (hipStream_t)hip_stream))) break;
                dsc = (const char *)d_scalars + submitted * sb;
            }
            if ((rc = vt->submit(*ctx, ws, dsc, n, rb.get()))) break;
            ++submitted;
        }
        if (rc) break;
        rc = vt->collect(*w[collected % nws], out_jac + collected * jl);
        ++collected;
    }
    for (size_t i = 0; i < nws; ++i) {
        (void)hipStreamSynchronize(w[i]->stream);  // nothing of this call is left running on a released workspace
        ctx->release(w[i]);
    }
    return rc;
}

GMSM_EXPORT int gmsm_multiexp_collect(uint64_t ticket, uint64_t *out_jac) {
    const unsigned slot = (unsigned)(ticket & 0xff), dev = (unsigned)(ticket >> 40);
    const uint32_t gen = (uint32_t)(ticket >> 8);
    Context *ctx = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_ctx_mu);
        if (dev < g_ctx.size()) ctx = g_ctx[dev];
    }
    if (!ctx || slot < 1 || slot > (unsigned)Context::NUM_WS) return fail(GMSM_ERR_ARG, "unknown MultiExp ticket");
    Workspace &ws = ctx->ws[slot - 1];
    const GroupVTable *vt;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        if (!ws.pending || ws.pending_gen != gen) return fail(GMSM_ERR_ARG, "unknown MultiExp ticket (already collected?)");
        ws.pending = false;  // claimed by this call; the workspace stays leased (busy) until the fold is done
        vt = vtable(ws.pending_group);
    }
    // The slot stays `pending` while we wait and fold, so nobody else touches it; the context lock is not held and the
    // other slot can be submitted to meanwhile.
    (void)hipSetDevice(ctx->device);
    int rc = vt->collect(ws, out_jac);
    ws.bases_ref.reset();
    ctx->release(&ws);
    return rc;
}

// ------------------------------------------------------------------ fr/fft
using FftRef = std::shared_ptr<FftDomain>;
static HandleTable<FftDomain> g_fft;

GMSM_EXPORT int gmsm_fft_domain_new(int group, uint64_t m, uint64_t *out_handle) {
    FR_OR_FAIL(group);
    if (!out_handle) return fail(GMSM_ERR_ARG, "gmsm_fft_domain_new: out_handle is null");
    unsigned log2n = 0;  // ecc.NextPowerOfTwo(m)
    while (log2n < 63 && ((uint64_t)1 << log2n) < m) ++log2n;
    Context *ctx;
    int rc = enter(&ctx);
    if (rc) return rc;
    GMSM_LEASE_OR_FAIL(lease, *ctx);
    FftRef d = std::make_shared<FftDomain>();
    d->group = group;
    d->device = ctx->device;
    if ((rc = vt->fft_domain_new(*ctx, lease.w->stream, log2n, d.get()))) return rc;
    *out_handle = g_fft.add(d);
    return GMSM_OK;
}

GMSM_EXPORT int gmsm_fft_domain_release(uint64_t handle) {
    if (!g_fft.take(handle)) return fail(GMSM_ERR_ARG, "unknown fft domain handle");  // the tables go with the last reference
    return GMSM_OK;
}

GMSM_EXPORT int gmsm_fft_domain_info(uint64_t handle, uint64_t *cardinality, uint64_t *generator, uint64_t *generator_inv,
                                     uint64_t *cardinality_inv, uint64_t *fr_multiplicative_gen,
                                     uint64_t *fr_multiplicative_gen_inv) {
    FftRef d = g_fft.get(handle);
    if (!d) return fail(GMSM_ERR_ARG, "unknown fft domain handle");
    if (cardinality) *cardinality = (uint64_t)1 << d->log2n;
    auto put = [](uint64_t *dst, const std::vector<uint64_t> &src) {
        if (dst) memcpy(dst, src.data(), src.size() * 8);
    };
    put(generator, d->generator);
    put(generator_inv, d->generator_inv);
    put(cardinality_inv, d->cardinality_inv);
    put(fr_multiplicative_gen, d->shift);
    put(fr_multiplicative_gen_inv, d->shift_inv);
    return GMSM_OK;
}

GMSM_EXPORT int gmsm_fft(uint64_t handle, uint64_t *a, void *d_a, size_t n, int inverse, int decimation, int on_coset,
                         void *hip_stream) {
    FftRef d = g_fft.get(handle);
    if (!d) return fail(GMSM_ERR_ARG, "unknown fft domain handle");
    const FieldVTable *vt = fr_vtable(d->group);
    if (n != ((size_t)1 << d->log2n)) return fail(GMSM_ERR_LEN, "len(a) must equal the domain's cardinality");
    if ((a == nullptr) == (d_a == nullptr)) return fail(GMSM_ERR_ARG, "gmsm_fft: give exactly one of a (host) / d_a (device)");
    if (decimation != 0 && decimation != 1) return fail(GMSM_ERR_ARG, "gmsm_fft: decimation must be 0 (DIT) or 1 (DIF)");
    Context *ctx;
    int rc = enter_on(d->device, &ctx);
    if (rc) return rc;
    GMSM_LEASE_OR_FAIL(lease, *ctx);
    Workspace &ws = *lease.w;
    const size_t bytes = n * vt->scalar_bytes;
    if (!a) {
        hipPointerAttribute_t attr;  // a vector on another GPU would fault (or read garbage) under this domain's tables
        if (hipPointerGetAttributes(&attr, d_a) != hipSuccess || attr.type != hipMemoryTypeDevice || attr.device != d->device) {
            (void)hipGetLastError();
            return fail(GMSM_ERR_ARG, "gmsm_fft: d_a is not device memory of the domain's device");
        }
    }
    void *dev;
    if ((rc = stage_input(ws, ws.h2d_scalars, a, d_a, bytes, {After::STREAM, (hipStream_t)hip_stream}, &dev))) return rc;
    {
        std::lock_guard<std::mutex> lk(d->mu);
        rc = vt->fft_run(ws.stream, d.get(), dev, inverse != 0, decimation == 1, on_coset != 0);
    }
    if (rc) return rc;
    if (a) HIP_TRY(hipMemcpyAsync(a, dev, bytes, hipMemcpyDeviceToHost, ws.stream));
    HIP_TRY(hipStreamSynchronize(ws.stream));
    return GMSM_OK;
}

GMSM_EXPORT int gmsm_fft_bit_reverse(int group, uint64_t *a, void *d_a, size_t n, void *hip_stream) {
    FR_OR_FAIL(group);
    if ((a == nullptr) == (d_a == nullptr) && n) return fail(GMSM_ERR_ARG, "gmsm_fft_bit_reverse: give exactly one of a / d_a");
    if (n == 0) return GMSM_OK;
    Context *ctx;
    int rc = enter_owner(d_a, &ctx);
    if (rc) return rc;
    GMSM_LEASE_OR_FAIL(lease, *ctx);
    Workspace &ws = *lease.w;
    const size_t bytes = n * vt->scalar_bytes;
    void *dev;
    if ((rc = stage_input(ws, ws.h2d_scalars, a, d_a, bytes, {After::STREAM, (hipStream_t)hip_stream}, &dev))) return rc;
    if ((rc = vt->fft_bit_reverse(ws.stream, dev, n))) return rc;
    if (a) HIP_TRY(hipMemcpyAsync(a, dev, bytes, hipMemcpyDeviceToHost, ws.stream));
    HIP_TRY(hipStreamSynchronize(ws.stream));
    return GMSM_OK;
}

// ------------------------------------------------------------------ KZG opening (gmsm_poly.h)
static const char *const ERR_POLY_SIZE = "invalid polynomial size (larger than SRS or == 0)";  // ErrInvalidPolynomialSize, kzg.go

// d must be 16-byte aligned device memory of `device` (a vector elsewhere would fault or read garbage)
static int check_device_vector(const char *entry, const char *name, const void *d, int device) {
    if (!d) return GMSM_OK;
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, d) != hipSuccess || attr.type != hipMemoryTypeDevice || attr.device != device) {
        (void)hipGetLastError();
        return fail(GMSM_ERR_ARG, std::string(entry) + ": " + name + " is not device memory of the call's device");
    }
    if ((uintptr_t)d % 16) return fail(GMSM_ERR_ARG, std::string(entry) + ": " + name + " is not 16-byte aligned");
    return GMSM_OK;
}

GMSM_EXPORT int gmsm_poly_eval(int group, const uint64_t *polys, const void *d_polys, const size_t *lens, size_t k,
                               const uint64_t *point, void *hip_stream, uint64_t *out_values) {
    FR_OR_FAIL(group);
    if (k == 0) return GMSM_OK;
    if (!lens || !point || !out_values) return fail(GMSM_ERR_ARG, "gmsm_poly_eval: lens, point and out_values must not be null");
    if ((polys == nullptr) == (d_polys == nullptr))
        return fail(GMSM_ERR_ARG, "gmsm_poly_eval: give exactly one of polys (host) / d_polys (device)");
    if (polys && polys == out_values) return fail(GMSM_ERR_ARG, "gmsm_poly_eval: out_values aliases polys (inputs are never modified)");
    for (size_t i = 0; i < k; ++i)
        if (lens[i] == 0) return fail(GMSM_ERR_ARG, "gmsm_poly_eval: polynomial " + std::to_string(i) + " is empty (eval reads p[len(p)-1])");
    Context *ctx;
    int rc = enter_owner(d_polys, &ctx);
    if (rc) return rc;
    if ((rc = check_device_vector("gmsm_poly_eval", "d_polys", d_polys, ctx->device))) return rc;
    return vt->poly_eval(*ctx, polys, d_polys, lens, k, point, (hipStream_t)hip_stream, out_values);
}

GMSM_EXPORT int gmsm_poly_div_x_minus_a(int group, const uint64_t *poly, const void *d_poly, size_t n, const uint64_t *point,
                                        void *hip_stream, uint64_t *out_h, void *d_out_h, uint64_t *out_value) {
    FR_OR_FAIL(group);
    const char *E = "gmsm_poly_div_x_minus_a";
    if (n == 0) return fail(GMSM_ERR_ARG, std::string(E) + ": n == 0 (f(a) of an empty polynomial is undefined)");
    if (!point) return fail(GMSM_ERR_ARG, std::string(E) + ": point is null");
    if ((poly == nullptr) == (d_poly == nullptr)) return fail(GMSM_ERR_ARG, std::string(E) + ": give exactly one of poly (host) / d_poly (device)");
    if (n > 1 && (out_h == nullptr) == (d_out_h == nullptr))
        return fail(GMSM_ERR_ARG, std::string(E) + ": give exactly one of out_h (host) / d_out_h (device)");
    if ((poly && (poly == out_h || poly == out_value)) || (d_poly && d_poly == d_out_h) || (out_h && out_h == out_value))
        return fail(GMSM_ERR_ARG, std::string(E) + ": an output aliases the input or another output (inputs are never modified)");
    Context *ctx;
    int rc = enter_owner(d_poly ? d_poly : d_out_h, &ctx);
    if (rc) return rc;
    if ((rc = check_device_vector(E, "d_poly", d_poly, ctx->device)) || (rc = check_device_vector(E, "d_out_h", n > 1 ? d_out_h : nullptr, ctx->device)))
        return rc;
    return vt->poly_div(*ctx, poly, d_poly, n, point, (hipStream_t)hip_stream, n > 1 ? out_h : nullptr, n > 1 ? d_out_h : nullptr, out_value);
}

// Open (kzg.go:180-205) and the part of BatchOpenSinglePoint after the challenge (:246-339) over registered bases
static int kzg_open_impl(const char *E, uint64_t handle, const uint64_t *polys, const void *d_polys, const size_t *lens, size_t k,
                         const uint64_t *point, const uint64_t *gamma, void *hip_stream, uint64_t *out_claimed, uint64_t *out_h_jac) {
    if (k == 0 || !lens) return fail(GMSM_ERR_ARG, std::string(E) + ": no polynomial");
    size_t maxlen = 0;
    for (size_t i = 0; i < k; ++i) {
        if (lens[i] == 0) return fail(GMSM_ERR_ARG, ERR_POLY_SIZE);
        maxlen = std::max(maxlen, lens[i]);
    }
    if (maxlen < 2) return fail(GMSM_ERR_ARG, ERR_POLY_SIZE);  // Commit of the empty quotient refuses it
    if (!point || !out_h_jac || (k > 1 && !gamma)) return fail(GMSM_ERR_ARG, std::string(E) + ": point, gamma and out_h_jac must not be null");
    if ((polys == nullptr) == (d_polys == nullptr)) return fail(GMSM_ERR_ARG, std::string(E) + ": give exactly one of polys (host) / d_polys (device)");
    if (out_claimed && (out_claimed == out_h_jac || out_claimed == polys))
        return fail(GMSM_ERR_ARG, std::string(E) + ": out_claimed aliases another argument");
    if (polys && polys == out_h_jac) return fail(GMSM_ERR_ARG, std::string(E) + ": out_h_jac aliases polys (inputs are never modified)");
    BasesRef rb = g_bases.get(handle);
    if (!rb) return fail(GMSM_ERR_ARG, "unknown bases handle");
    if (maxlen > rb->n) return fail(GMSM_ERR_ARG, ERR_POLY_SIZE);
    const GroupVTable *vt = vtable(rb->group);
    Context *ctx;
    int rc = enter_on(rb->device, &ctx);  // the bases decide the device
    if (rc) return rc;
    if ((rc = check_device_vector(E, "d_polys", d_polys, ctx->device))) return rc;
    return vt->kzg_open(*ctx, polys, d_polys, lens, k, point, k > 1 ? gamma : nullptr, (hipStream_t)hip_stream, out_claimed, out_h_jac,
                        rb.get());
}

GMSM_EXPORT int gmsm_kzg_open(uint64_t handle, const uint64_t *poly, const void *d_poly, size_t n, const uint64_t *point,
                              void *hip_stream, uint64_t *out_claimed, uint64_t *out_h_jac) {
    if (!out_claimed) return fail(GMSM_ERR_ARG, "gmsm_kzg_open: out_claimed is null");
    return kzg_open_impl("gmsm_kzg_open", handle, poly, d_poly, &n, 1, point, nullptr, hip_stream, out_claimed, out_h_jac);
}

GMSM_EXPORT int gmsm_kzg_open_folded(uint64_t handle, const uint64_t *polys, const void *d_polys, const size_t *lens, size_t k,
                                     const uint64_t *point, const uint64_t *gamma, void *hip_stream, uint64_t *out_h_jac) {
    return kzg_open_impl("gmsm_kzg_open_folded", handle, polys, d_polys, lens, k, point, gamma, hip_stream, nullptr, out_h_jac);
}

// ------------------------------------------------------------------ shplonk.BatchOpen, fflonk.BatchOpen (gmsm_fflonk.h)
static const char *const ERR_SHPLONK_G1 = "shplonk opens over G1 bases only";
static const char *const ERR_FFLONK_G1 = "fflonk commits and opens over G1 bases only";

// The four open entries take shplonk's k polynomials (pack_sizes is no argument of theirs: null from here on) or fflonk's k
// packs. Their checks, in this order: the counts and arrays (open_nonempty), the entry's own pointers and aliases, then
// open_check: the polynomials' pointer pair, the handle, G1, every refusal that depends on the polynomials and the points
// (FieldVTable::open_check: shplonk.go:44-83, fflonk.go:77-141), the size condition last - the reference commits w' over
// maxSizePolys + sum_i npoints[i] - 1 coefficients, so that many bases must be registered although the device MSMs run over
// true lengths only (kzg.go:159-162) - all on the host, then the device of the bases.
static int open_nonempty(const char *E, bool packed, const size_t *lens, const size_t *pack_sizes, size_t k, const uint64_t *points,
                         const size_t *npoints) {
    if (k == 0 || !lens || (packed && !pack_sizes) || !npoints || !points)
        return fail(GMSM_ERR_ARG, std::string(E) + (packed ? ": no pack of polynomials, or lens / pack_sizes / points / npoints is null"
                                                           : ": no polynomial, or lens / points / npoints is null"));
    return GMSM_OK;
}

static int open_check(const char *E, uint64_t handle, const uint64_t *polys, const void *d_polys, const size_t *lens, const size_t *pack_sizes,
                      size_t k, const uint64_t *points, const size_t *npoints, BasesRef *rb_out, const GroupVTable **vt_out, Context **ctx_out) {
    if ((polys == nullptr) == (d_polys == nullptr)) return fail(GMSM_ERR_ARG, std::string(E) + ": give exactly one of polys (host) / d_polys (device)");
    BasesRef rb = g_bases.get(handle);
    if (!rb) return fail(GMSM_ERR_ARG, "unknown bases handle");
    const GroupVTable *vt = vtable(rb->group);
    if (!vt->open_w) return fail(GMSM_ERR_ARG, pack_sizes ? ERR_FFLONK_G1 : ERR_SHPLONK_G1);
    int rc = fr_vtable(rb->group)->open_check(E, lens, pack_sizes, k, points, npoints, true, rb->n);
    if (rc) return rc;
    Context *ctx;
    if ((rc = enter_on(rb->device, &ctx))) return rc;  // the bases decide the device
    if ((rc = check_device_vector(E, "d_polys", d_polys, ctx->device))) return rc;
    *rb_out = rb, *vt_out = vt, *ctx_out = ctx;
    return GMSM_OK;
}

GMSM_EXPORT int gmsm_shplonk_open_w(uint64_t handle, const uint64_t *polys, const void *d_polys, const size_t *lens, size_t k,
                                    const uint64_t *points, const size_t *npoints, const uint64_t *gamma, void *hip_stream,
                                    uint64_t *out_claimed, uint64_t *out_w, void *d_out_w, uint64_t *out_w_jac) {
    const char *E = "gmsm_shplonk_open_w";
    if (int rc0 = open_nonempty(E, false, lens, nullptr, k, points, npoints)) return rc0;
    if (!gamma || !out_claimed || !out_w_jac) return fail(GMSM_ERR_ARG, std::string(E) + ": gamma, out_claimed and out_w_jac must not be null");
    if ((out_w == nullptr) == (d_out_w == nullptr)) return fail(GMSM_ERR_ARG, std::string(E) + ": give exactly one of out_w (host) / d_out_w (device)");
    if ((polys && (polys == out_w || polys == out_claimed || polys == out_w_jac)) || (d_polys && d_polys == d_out_w) || out_claimed == out_w ||
        out_claimed == out_w_jac || out_w == out_w_jac || points == out_claimed || points == out_w)
        return fail(GMSM_ERR_ARG, std::string(E) + ": an output aliases an input or another output (inputs are never modified)");
    BasesRef rb;
    const GroupVTable *vt;
    Context *ctx;
    int rc = open_check(E, handle, polys, d_polys, lens, nullptr, k, points, npoints, &rb, &vt, &ctx);
    if (rc) return rc;
    if ((rc = check_device_vector(E, "d_out_w", d_out_w, ctx->device))) return rc;
    return vt->open_w(*ctx, polys, d_polys, lens, nullptr, k, points, npoints, gamma, (hipStream_t)hip_stream, out_claimed, nullptr, out_w,
                      d_out_w, out_w_jac, rb.get());
}

GMSM_EXPORT int gmsm_shplonk_open_wprime(uint64_t handle, const uint64_t *polys, const void *d_polys, const size_t *lens, size_t k,
                                         const uint64_t *points, const size_t *npoints, const uint64_t *claimed, const uint64_t *gamma,
                                         const uint64_t *w, const void *d_w, const uint64_t *z, void *hip_stream, uint64_t *out_wprime_jac) {
    const char *E = "gmsm_shplonk_open_wprime";
    if (int rc0 = open_nonempty(E, false, lens, nullptr, k, points, npoints)) return rc0;
    if (!claimed || !gamma || !z || !out_wprime_jac)
        return fail(GMSM_ERR_ARG, std::string(E) + ": claimed, gamma, z and out_wprime_jac must not be null");
    if ((w == nullptr) == (d_w == nullptr)) return fail(GMSM_ERR_ARG, std::string(E) + ": give exactly one of w (host) / d_w (device)");
    if ((polys && polys == out_wprime_jac) || (w && w == out_wprime_jac) || points == out_wprime_jac || claimed == out_wprime_jac)
        return fail(GMSM_ERR_ARG, std::string(E) + ": out_wprime_jac aliases an input (inputs are never modified)");
    BasesRef rb;
    const GroupVTable *vt;
    Context *ctx;
    int rc = open_check(E, handle, polys, d_polys, lens, nullptr, k, points, npoints, &rb, &vt, &ctx);
    if (rc) return rc;
    if ((rc = check_device_vector(E, "d_w", d_w, ctx->device))) return rc;
    return vt->open_wprime(*ctx, polys, d_polys, lens, nullptr, k, points, npoints, claimed, gamma, w, d_w, z, (hipStream_t)hip_stream,
                           out_wprime_jac, rb.get());
}

// ------------------------------------------------------------------ fflonk Fold, FoldAndCommit, BatchOpen (gmsm_fflonk.h)

GMSM_EXPORT int gmsm_fflonk_next_divisor(int group, size_t n, size_t *out_t) {
    FR_OR_FAIL(group);
    const char *E = "gmsm_fflonk_next_divisor";
    if (!out_t) return fail(GMSM_ERR_ARG, std::string(E) + ": out_t is null");
    if (n == 0) return fail(GMSM_ERR_ARG, std::string(E) + ": n == 0");
    if (!vt->fflonk_next_divisor(n, out_t))
        return fail(GMSM_ERR_ARG, std::string(E) + ": did not find any divisor of r-1 within 100 trials above " + std::to_string(n));
    return GMSM_OK;
}

// One pack for Fold / FoldAndCommit: the pointer checks, then the pack's own (host only)
static int fflonk_pack_args(const char *E, const uint64_t *polys, const void *d_polys, const size_t *lens, size_t npolys) {
    if (npolys == 0 || !lens) return fail(GMSM_ERR_ARG, std::string(E) + ": no polynomial, or lens is null");
    if ((polys == nullptr) == (d_polys == nullptr)) return fail(GMSM_ERR_ARG, std::string(E) + ": give exactly one of polys (host) / d_polys (device)");
    return GMSM_OK;
}

GMSM_EXPORT int gmsm_fflonk_fold(int group, const uint64_t *polys, const void *d_polys, const size_t *lens, size_t npolys, void *hip_stream,
                                 uint64_t *out, void *d_out) {
    VT_OR_FAIL(group);
    const char *E = "gmsm_fflonk_fold";
    if ((out == nullptr) == (d_out == nullptr)) return fail(GMSM_ERR_ARG, std::string(E) + ": give exactly one of out (host) / d_out (device)");
    if ((polys && polys == out) || (d_polys && d_polys == d_out))
        return fail(GMSM_ERR_ARG, std::string(E) + ": the output aliases the input (inputs are never modified)");
    int rc = fflonk_pack_args(E, polys, d_polys, lens, npolys);
    if (rc || (rc = fr_vtable(group)->open_check(E, lens, &npolys, 1, nullptr, nullptr, false, 0))) return rc;
    Context *ctx;
    if ((rc = enter_owner(d_polys ? d_polys : d_out, &ctx))) return rc;
    if ((rc = check_device_vector(E, "d_polys", d_polys, ctx->device)) || (rc = check_device_vector(E, "d_out", d_out, ctx->device))) return rc;
    return vt->fflonk_fold(*ctx, polys, d_polys, lens, npolys, (hipStream_t)hip_stream, out, d_out, nullptr, nullptr);
}

GMSM_EXPORT int gmsm_fflonk_fold_commit(uint64_t handle, const uint64_t *polys, const void *d_polys, const size_t *lens, size_t npolys,
                                        void *hip_stream, void *d_out_folded, uint64_t *out_jac) {
    const char *E = "gmsm_fflonk_fold_commit";
    if (!out_jac) return fail(GMSM_ERR_ARG, std::string(E) + ": out_jac is null");
    if ((polys && polys == out_jac) || (d_polys && d_polys == d_out_folded))
        return fail(GMSM_ERR_ARG, std::string(E) + ": an output aliases the input (inputs are never modified)");
    int rc = fflonk_pack_args(E, polys, d_polys, lens, npolys);
    if (rc) return rc;
    BasesRef rb = g_bases.get(handle);
    if (!rb) return fail(GMSM_ERR_ARG, "unknown bases handle");
    const GroupVTable *vt = vtable(rb->group);
    if (!vt->open_w) return fail(GMSM_ERR_ARG, ERR_FFLONK_G1);
    if ((rc = fr_vtable(rb->group)->open_check(E, lens, &npolys, 1, nullptr, nullptr, false, 0))) return rc;
    size_t t = 0, n = 0;
    fr_vtable(rb->group)->fflonk_next_divisor(npolys, &t);
    for (size_t j = 0; j < npolys; ++j) n = std::max(n, lens[j]);
    if (t * n > rb->n) return fail(GMSM_ERR_ARG, ERR_POLY_SIZE);  // Commit's size check (kzg.go:159-162) over the folded length
    Context *ctx;
    if ((rc = enter_on(rb->device, &ctx))) return rc;  // the bases decide the device
    if ((rc = check_device_vector(E, "d_polys", d_polys, ctx->device)) || (rc = check_device_vector(E, "d_out_folded", d_out_folded, ctx->device)))
        return rc;
    return vt->fflonk_fold(*ctx, polys, d_polys, lens, npolys, (hipStream_t)hip_stream, nullptr, d_out_folded, rb.get(), out_jac);
}

GMSM_EXPORT int gmsm_fflonk_open_w(uint64_t handle, const uint64_t *polys, const void *d_polys, const size_t *lens, const size_t *pack_sizes,
                                   size_t k, const uint64_t *points, const size_t *npoints, const uint64_t *gamma, void *hip_stream,
                                   uint64_t *out_claimed, uint64_t *out_folded_claimed, uint64_t *out_w, void *d_out_w, uint64_t *out_w_jac) {
    const char *E = "gmsm_fflonk_open_w";
    if (int rc0 = open_nonempty(E, true, lens, pack_sizes, k, points, npoints)) return rc0;
    if (!gamma || !out_claimed || !out_folded_claimed || !out_w_jac)
        return fail(GMSM_ERR_ARG, std::string(E) + ": gamma, out_claimed, out_folded_claimed and out_w_jac must not be null");
    if ((out_w == nullptr) == (d_out_w == nullptr)) return fail(GMSM_ERR_ARG, std::string(E) + ": give exactly one of out_w (host) / d_out_w (device)");
    const uint64_t *outs[] = {out_claimed, out_folded_claimed, out_w, out_w_jac};
    bool alias = d_polys && d_polys == d_out_w;
    for (int a = 0; a < 4; ++a) {
        if (!outs[a]) continue;
        alias = alias || outs[a] == polys || outs[a] == points || outs[a] == gamma;
        for (int b = a + 1; b < 4; ++b) alias = alias || outs[a] == outs[b];
    }
    if (alias) return fail(GMSM_ERR_ARG, std::string(E) + ": an output aliases an input or another output (inputs are never modified)");
    BasesRef rb;
    const GroupVTable *vt;
    Context *ctx;
    int rc = open_check(E, handle, polys, d_polys, lens, pack_sizes, k, points, npoints, &rb, &vt, &ctx);
    if (rc) return rc;
    if ((rc = check_device_vector(E, "d_out_w", d_out_w, ctx->device))) return rc;
    return vt->open_w(*ctx, polys, d_polys, lens, pack_sizes, k, points, npoints, gamma, (hipStream_t)hip_stream, out_claimed,
                      out_folded_claimed, out_w, d_out_w, out_w_jac, rb.get());
}

GMSM_EXPORT int gmsm_fflonk_open_wprime(uint64_t handle, const uint64_t *polys, const void *d_polys, const size_t *lens,
                                        const size_t *pack_sizes, size_t k, const uint64_t *points, const size_t *npoints,
                                        const uint64_t *folded_claimed, const uint64_t *gamma, const uint64_t *w, const void *d_w,
                                        const uint64_t *z, void *hip_stream, uint64_t *out_wprime_jac) {
    const char *E = "gmsm_fflonk_open_wprime";
    if (int rc0 = open_nonempty(E, true, lens, pack_sizes, k, points, npoints)) return rc0;
    if (!folded_claimed || !gamma || !z || !out_wprime_jac)
        return fail(GMSM_ERR_ARG, std::string(E) + ": folded_claimed, gamma, z and out_wprime_jac must not be null");
    if ((w == nullptr) == (d_w == nullptr)) return fail(GMSM_ERR_ARG, std::string(E) + ": give exactly one of w (host) / d_w (device)");
    if ((polys && polys == out_wprime_jac) || (w && w == out_wprime_jac) || points == out_wprime_jac || folded_claimed == out_wprime_jac)
        return fail(GMSM_ERR_ARG, std::string(E) + ": out_wprime_jac aliases an input (inputs are never modified)");
    BasesRef rb;
    const GroupVTable *vt;
    Context *ctx;
    int rc = open_check(E, handle, polys, d_polys, lens, pack_sizes, k, points, npoints, &rb, &vt, &ctx);
    if (rc) return rc;
    if ((rc = check_device_vector(E, "d_w", d_w, ctx->device))) return rc;
    return vt->open_wprime(*ctx, polys, d_polys, lens, pack_sizes, k, points, npoints, folded_claimed, gamma, w, d_w, z,
                           (hipStream_t)hip_stream, out_wprime_jac, rb.get());
}

// ------------------------------------------------------------------ ToLagrangeG1 (gmsm_group_fft.h)
static const char *const ERR_POW2 = "len(coeffs) must be a power of 2";  // ToLagrangeG1, kzg/utils.go
static const char *const ERR_G1_ONLY = "ToLagrangeG1 is defined for G1 only";
static const char *const ERR_ROOT = "m is too big: the required root of unity does not exist";  // as gmsm_fft_domain_new

// the size checks of ToLagrangeG1 and computeTwiddlesInv (fr.Generator): no device needed
static int lagrange_size(const FieldVTable *vt, size_t n, unsigned *log2n) {
    if (n == 0 || (n & (n - 1))) return fail(GMSM_ERR_ARG, ERR_POW2);
    unsigned l = 0;
    while (((size_t)1 << l) < n) ++l;
    if (l > vt->fr_max_order) return fail(GMSM_ERR_ARG, ERR_ROOT);
    *log2n = l;
    return GMSM_OK;
}

GMSM_EXPORT int gmsm_to_lagrange_g1(int group, const uint64_t *coeffs, const void *d_coeffs, size_t n, void *hip_stream,
                                    uint64_t *out_affine, void *d_out_affine) {
    VT_OR_FAIL(group);
    const char *E = "gmsm_to_lagrange_g1";
    if (!vt->to_lagrange) return fail(GMSM_ERR_ARG, ERR_G1_ONLY);
    unsigned log2n;
    int rc = lagrange_size(fr_vtable(group), n, &log2n);
    if (rc) return rc;
    if ((coeffs == nullptr) == (d_coeffs == nullptr)) return fail(GMSM_ERR_ARG, std::string(E) + ": give exactly one of coeffs (host) / d_coeffs (device)");
    if ((out_affine == nullptr) == (d_out_affine == nullptr))
        return fail(GMSM_ERR_ARG, std::string(E) + ": give exactly one of out_affine (host) / d_out_affine (device)");
    Context *ctx;
    if ((rc = enter_owner(d_coeffs ? d_coeffs : d_out_affine, &ctx))) return rc;
    if ((rc = check_device_vector(E, "d_coeffs", d_coeffs, ctx->device)) || (rc = check_device_vector(E, "d_out_affine", d_out_affine, ctx->device)))
        return rc;
    return vt->to_lagrange(*ctx, coeffs, d_coeffs, nullptr, log2n, (hipStream_t)hip_stream, out_affine, d_out_affine, nullptr);
}

GMSM_EXPORT int gmsm_bases_to_lagrange(uint64_t handle, size_t n, uint64_t *out_handle) {
    if (!out_handle) return fail(GMSM_ERR_ARG, "gmsm_bases_to_lagrange: out_handle is null");
    BasesRef rb = g_bases.get(handle);
    if (!rb) return fail(GMSM_ERR_ARG, "unknown bases handle");
    const GroupVTable *vt = vtable(rb->group);
    if (!vt->to_lagrange) return fail(GMSM_ERR_ARG, ERR_G1_ONLY);
    unsigned log2n;
    int rc = lagrange_size(fr_vtable(rb->group), n, &log2n);
    if (rc) return rc;
    if (n > rb->n) return fail(GMSM_ERR_ARG, "gmsm_bases_to_lagrange: n is larger than the registered bases");
    Context *ctx;
    if ((rc = enter_on(rb->device, &ctx))) return rc;  // the bases decide the device
    BasesRef out = std::make_shared<ResidentBases>();
    out->group = rb->group;
    out->device = ctx->device;
    if ((rc = vt->to_lagrange(*ctx, nullptr, nullptr, rb.get(), log2n, nullptr, nullptr, nullptr, out.get()))) return rc;
    *out_handle = g_bases.add(out);
    return GMSM_OK;
}

// ------------------------------------------------------------------ mpcsetup updates (gmsm_scale.h)
// the pointer pairs of the two batch entries, then the call through the vtable
static int scale_call(const char *E, const GroupVTable *vt, const uint64_t *points, const void *d_points, size_t n, const uint64_t *scalars,
                      const void *d_scalars, size_t n_scalars, const uint64_t *r, void *hip_stream, uint64_t *out_affine, void *d_out_affine) {
    if ((points == nullptr) == (d_points == nullptr)) return fail(GMSM_ERR_ARG, std::string(E) + ": give exactly one of points (host) / d_points (device)");
    if (!r && (scalars == nullptr) == (d_scalars == nullptr))
        return fail(GMSM_ERR_ARG, std::string(E) + ": give exactly one of scalars (host) / d_scalars (device)");
    if ((out_affine == nullptr) == (d_out_affine == nullptr))
        return fail(GMSM_ERR_ARG, std::string(E) + ": give exactly one of out_affine (host) / d_out_affine (device)");
    Context *ctx;
    int rc = enter_owner(d_points ? d_points : d_out_affine ? d_out_affine : d_scalars, &ctx);
    if (rc) return rc;
    if ((rc = check_device_vector(E, "d_points", d_points, ctx->device)) || (rc = check_device_vector(E, "d_scalars", d_scalars, ctx->device)) ||
        (rc = check_device_vector(E, "d_out_affine", d_out_affine, ctx->device)))
        return rc;
    return vt->batch_scale(*ctx, points, d_points, n, scalars, d_scalars, n_scalars, r, (hipStream_t)hip_stream, out_affine, d_out_affine);
}

GMSM_EXPORT int gmsm_batch_scale(int group, const uint64_t *points, const void *d_points, size_t n, const uint64_t *scalars,
                                 const void *d_scalars, size_t n_scalars, void *hip_stream, uint64_t *out_affine, void *d_out_affine) {
    VT_OR_FAIL(group);
    if (n_scalars != n && n_scalars != 1) return fail(GMSM_ERR_LEN, "gmsm_batch_scale: n_scalars must be n (one scalar per point) or 1 (one for all)");
    if (n == 0) return GMSM_OK;
    return scale_call("gmsm_batch_scale", vt, points, d_points, n, scalars, d_scalars, n_scalars, nullptr, hip_stream, out_affine, d_out_affine);
}

GMSM_EXPORT int gmsm_update_monomials(int group, const uint64_t *points, const void *d_points, size_t n, const uint64_t *r, void *hip_stream,
                                      uint64_t *out_affine, void *d_out_affine) {
    VT_OR_FAIL(group);
    if (n < 2) return fail(GMSM_ERR_ARG, "gmsm_update_monomials: needs at least 2 points (UpdateMonomialsG1 starts at A[1])");
    if (!r) return fail(GMSM_ERR_ARG, "gmsm_update_monomials: r is null");
    return scale_call("gmsm_update_monomials", vt, points, d_points, n, nullptr, nullptr, 0, r, hip_stream, out_affine, d_out_affine);
}

GMSM_EXPORT int gmsm_linear_combinations(int group, const uint64_t *points, const void *d_points, size_t n, const size_t *ends, size_t n_ends,
                                         const uint64_t *r, void *hip_stream, uint64_t *out_truncated_jac, uint64_t *out_shifted_jac) {
    VT_OR_FAIL(group);
    const char *E = "gmsm_linear_combinations";
    if ((points == nullptr) == (d_points == nullptr)) return fail(GMSM_ERR_ARG, std::string(E) + ": give exactly one of points (host) / d_points (device)");
    if (!ends || !n_ends || !r || !out_truncated_jac || !out_shifted_jac)
        return fail(GMSM_ERR_ARG, std::string(E) + ": ends, r, out_truncated_jac and out_shifted_jac must not be null, n_ends not 0");
    for (size_t j = 0, prev = 0; j < n_ends; prev = ends[j], ++j) {
        if (ends[j] <= prev) return fail(GMSM_ERR_ARG, std::string(E) + ": ends must be strictly increasing");
        if (ends[j] - prev < 2) return fail(GMSM_ERR_ARG, "each slice must be of length at least 2");
    }
    if (ends[n_ends - 1] != n) return fail(GMSM_ERR_ARG, "lengths mismatch");
    Context *ctx;
    int rc = enter_owner(d_points, &ctx);
    if (rc) return rc;
    if ((rc = check_device_vector(E, "d_points", d_points, ctx->device))) return rc;
    return vt->linear_combinations(*ctx, points, d_points, n, ends, n_ends, r, (hipStream_t)hip_stream, out_truncated_jac, out_shifted_jac);
}

// ------------------------------------------------------------------ fr.BatchInvert, iop ratio polynomials (gmsm_ratio.h)
GMSM_EXPORT int gmsm_fr_batch_invert(int group, const uint64_t *a, const void *d_a, size_t n, void *hip_stream, uint64_t *out, void *d_out) {
    FR_OR_FAIL(group);
    const char *E = "gmsm_fr_batch_invert";
    if (n == 0) return GMSM_OK;
    if ((a == nullptr) == (d_a == nullptr)) return fail(GMSM_ERR_ARG, std::string(E) + ": give exactly one of a (host) / d_a (device)");
    if ((out == nullptr) == (d_out == nullptr)) return fail(GMSM_ERR_ARG, std::string(E) + ": give exactly one of out (host) / d_out (device)");
    Context *ctx;
    int rc = enter_owner(d_a ? d_a : d_out, &ctx);
    if (rc) return rc;
    if ((rc = check_device_vector(E, "d_a", d_a, ctx->device)) || (rc = check_device_vector(E, "d_out", d_out, ctx->device))) return rc;
    return vt->fr_batch_invert(*ctx, a, d_a, n, (hipStream_t)hip_stream, out, d_out);
}

// The host checks of the two ratio entries, in this order: what needs nothing but the arguments - the count, the expected form,
// the output pair (ratio_form), then the entry's own pointers, pairs and layout values - then the domain handle (ratio_domain),
// then what needs the domain's cardinality: the overlap of the output with an input, the range of a host permutation.
static int ratio_form(const char *E, size_t m, int basis, int layout, uint64_t *out, void *d_out) {
    if (m == 0) return fail(GMSM_ERR_ARG, std::string(E) + ": no polynomial (m == 0)");
    if (basis != 1 && basis != 2 && basis != 4)
        return fail(GMSM_ERR_ARG, std::string(E) + ": unknown basis " + std::to_string(basis) + " (1 Canonical, 2 Lagrange, 4 LagrangeCoset)");
    if (layout != 8 && layout != 16)
        return fail(GMSM_ERR_ARG, std::string(E) + ": unknown layout " + std::to_string(layout) + " (8 Regular, 16 BitReverse)");
    if ((out == nullptr) == (d_out == nullptr)) return fail(GMSM_ERR_ARG, std::string(E) + ": give exactly one of out (host) / d_out (device)");
    return GMSM_OK;
}
static int ratio_layouts(const char *E, const char *name, const uint32_t *layouts, size_t m) {
    if (!layouts) return fail(GMSM_ERR_ARG, std::string(E) + ": " + name + " is null");
    for (size_t j = 0; j < m; ++j)
        if (layouts[j] != 8 && layouts[j] != 16)
            return fail(GMSM_ERR_ARG, std::string(E) + ": " + name + "[" + std::to_string(j) + "] = " + std::to_string(layouts[j]) +
                                          " is no layout (8 Regular, 16 BitReverse)");
    return GMSM_OK;
}
static int ratio_pair(const char *E, const char *host, const char *dev, const void *h, const void *d) {
    if ((h == nullptr) == (d == nullptr))
        return fail(GMSM_ERR_ARG, std::string(E) + ": give exactly one of " + host + " (host) / " + dev + " (device)");
    return GMSM_OK;
}
static int ratio_domain(const char *E, uint64_t domain, size_t m, FftRef *d_out_ref, const FieldVTable **vt_out) {
    FftRef d = g_fft.get(domain);
    if (!d) return fail(GMSM_ERR_ARG, "unknown fft domain handle");
    if (m > (((size_t)1 << 62) >> d->log2n)) return fail(GMSM_ERR_ARG, std::string(E) + ": m * n does not fit");
    *d_out_ref = d, *vt_out = fr_vtable(d->group);
    return GMSM_OK;
}
// the output (host or device, out_bytes) shares a byte with an input vector of in_bytes on the same side
static bool ratio_overlap(const void *out, const void *d_out, size_t out_bytes, const void *in, const void *d_in, size_t in_bytes) {
    const uintptr_t o = (uintptr_t)(out ? out : d_out), i = (uintptr_t)(out ? in : d_in);
    return i != 0 && o < i + in_bytes && i < o + out_bytes;
}
static int ratio_aliases(const char *E) { return fail(GMSM_ERR_ARG, std::string(E) + ": the output overlaps an input (inputs are never modified)"); }

GMSM_EXPORT int gmsm_iop_ratio_copy_constraint(uint64_t domain, const uint64_t *entries, const void *d_entries, size_t m, const uint32_t *layouts,
                                               const int64_t *perm, const void *d_perm, const uint64_t *beta, const uint64_t *gamma, int basis,
                                               int layout, void *hip_stream, uint64_t *out, void *d_out) {
    const char *E = "gmsm_iop_ratio_copy_constraint";
    int rc = ratio_form(E, m, basis, layout, out, d_out);
    if (rc || (rc = ratio_layouts(E, "layouts", layouts, m))) return rc;
    if (!beta || !gamma) return fail(GMSM_ERR_ARG, std::string(E) + ": beta and gamma must not be null");
    if ((rc = ratio_pair(E, "entries", "d_entries", entries, d_entries)) || (rc = ratio_pair(E, "perm", "d_perm", perm, d_perm))) return rc;
    FftRef d;
    const FieldVTable *vt;
    if ((rc = ratio_domain(E, domain, m, &d, &vt))) return rc;
    const size_t mn = m << d->log2n, zbytes = vt->scalar_bytes << d->log2n;
    if (ratio_overlap(out, d_out, zbytes, entries, d_entries, m * zbytes) || ratio_overlap(out, d_out, zbytes, perm, d_perm, mn * 8))
        return ratio_aliases(E);
    if (perm)  // a permutation on the device is checked by the factor kernel
        for (size_t i = 0; i < mn; ++i)
            if (perm[i] < 0 || (uint64_t)perm[i] >= mn) return fail(GMSM_ERR_ARG, ratio_perm_error(i, perm[i], mn));
    Context *ctx;
    if ((rc = enter_on(d->device, &ctx))) return rc;  // the domain decides the device
    if ((rc = check_device_vector(E, "d_entries", d_entries, ctx->device)) || (rc = check_device_vector(E, "d_perm", d_perm, ctx->device)) ||
        (rc = check_device_vector(E, "d_out", d_out, ctx->device)))
        return rc;
    return vt->ratio_copy(*ctx, d.get(), entries, d_entries, m, layouts, perm, d_perm, beta, gamma, basis, layout, (hipStream_t)hip_stream, out, d_out);
}

GMSM_EXPORT int gmsm_iop_ratio_shuffled(uint64_t domain, const uint64_t *num, const void *d_num, const uint64_t *den, const void *d_den, size_t m,
                                        const uint32_t *num_layouts, const uint32_t *den_layouts, const uint64_t *beta, int basis, int layout,
                                        void *hip_stream, uint64_t *out, void *d_out) {
    const char *E = "gmsm_iop_ratio_shuffled";
    int rc = ratio_form(E, m, basis, layout, out, d_out);
    if (rc || (rc = ratio_layouts(E, "num_layouts", num_layouts, m)) || (rc = ratio_layouts(E, "den_layouts", den_layouts, m))) return rc;
    if (!beta) return fail(GMSM_ERR_ARG, std::string(E) + ": beta must not be null");
    if ((rc = ratio_pair(E, "num", "d_num", num, d_num)) || (rc = ratio_pair(E, "den", "d_den", den, d_den))) return rc;
    FftRef d;
    const FieldVTable *vt;
    if ((rc = ratio_domain(E, domain, m, &d, &vt))) return rc;
    const size_t zbytes = vt->scalar_bytes << d->log2n;
    if (ratio_overlap(out, d_out, zbytes, num, d_num, m * zbytes) || ratio_overlap(out, d_out, zbytes, den, d_den, m * zbytes)) return ratio_aliases(E);
    Context *ctx;
    if ((rc = enter_on(d->device, &ctx))) return rc;  // the domain decides the device
    if ((rc = check_device_vector(E, "d_num", d_num, ctx->device)) || (rc = check_device_vector(E, "d_den", d_den, ctx->device)) ||
        (rc = check_device_vector(E, "d_out", d_out, ctx->device)))
        return rc;
    return vt->ratio_shuffled(*ctx, d.get(), num, d_num, den, d_den, m, num_layouts, den_layouts, beta, basis, layout, (hipStream_t)hip_stream, out,
                              d_out);
}

// ------------------------------------------------------------------ iop.Polynomial: basis changes, Evaluate, DivideByXMinusOne (gmsm_iop_poly.h)
// Checks in the order of the ratio entries: what needs nothing but the arguments, then the domain handles, then what needs
// their cardinalities.
static int iop_basis(const char *E, const char *name, int basis) {
    if (basis != 1 && basis != 2 && basis != 4)
        return fail(GMSM_ERR_ARG, std::string(E) + ": unknown " + name + " " + std::to_string(basis) + " (1 Canonical, 2 Lagrange, 4 LagrangeCoset)");
    return GMSM_OK;
}
static int iop_layout(const char *E, int layout) {
    if (layout != 8 && layout != 16)
        return fail(GMSM_ERR_ARG, std::string(E) + ": unknown layout " + std::to_string(layout) + " (8 Regular, 16 BitReverse)");
    return GMSM_OK;
}

GMSM_EXPORT int gmsm_iop_to_basis(uint64_t domain, uint64_t *a, void *d_a, size_t len, int basis, int layout, int to_basis, void *hip_stream,
                                  int *out_layout) {
    const char *E = "gmsm_iop_to_basis";
    int rc = ratio_pair(E, "a", "d_a", a, d_a);
    if (rc || (rc = iop_basis(E, "basis", basis)) || (rc = iop_layout(E, layout)) || (rc = iop_basis(E, "to_basis", to_basis))) return rc;
    if (!out_layout) return fail(GMSM_ERR_ARG, std::string(E) + ": out_layout is null");
    FftRef d = g_fft.get(domain);
    if (!d) return fail(GMSM_ERR_ARG, "unknown fft domain handle");
    if (len > ((size_t)1 << d->log2n))
        return fail(GMSM_ERR_ARG, std::string(E) + ": len " + std::to_string(len) + " is larger than the domain's cardinality");
    const FieldVTable *vt = fr_vtable(d->group);
    Context *ctx;
    if ((rc = enter_on(d->device, &ctx))) return rc;  // the domain decides the device
    if ((rc = check_device_vector(E, "d_a", d_a, ctx->device))) return rc;
    return vt->iop_to_basis(*ctx, d.get(), a, d_a, len, basis, layout, to_basis, (hipStream_t)hip_stream, out_layout);
}

GMSM_EXPORT int gmsm_iop_evaluate(int group, const uint64_t *polys, const void *d_polys, size_t k, size_t len, size_t size, int basis,
                                  const uint32_t *layouts, unsigned shift, const uint64_t *coset, const uint64_t *x, void *hip_stream,
                                  uint64_t *out_values) {
    FR_OR_FAIL(group);
    const char *E = "gmsm_iop_evaluate";
    if (k == 0) return fail(GMSM_ERR_ARG, std::string(E) + ": no polynomial (k == 0)");
    if (len == 0) return fail(GMSM_ERR_ARG, std::string(E) + ": empty polynomial (len == 0)");
    if (size == 0) return fail(GMSM_ERR_ARG, std::string(E) + ": size == 0");
    int rc = iop_basis(E, "basis", basis);
    if (rc || (rc = ratio_layouts(E, "layouts", layouts, k)) || (rc = ratio_pair(E, "polys", "d_polys", polys, d_polys))) return rc;
    if (!x || !out_values) return fail(GMSM_ERR_ARG, std::string(E) + ": x and out_values must not be null");
    if (basis == 4 && !coset) return fail(GMSM_ERR_ARG, std::string(E) + ": coset is null and the basis is LagrangeCoset");
    if (shift > 5)
        return fail(GMSM_ERR_ARG, std::string(E) + ": shift " + std::to_string(shift) + " is outside 0..5 (the reference evaluates at 0 there)");
    bool reversed = false;
    for (size_t j = 0; j < k; ++j) reversed = reversed || layouts[j] == 16;
    if ((basis != 1 || reversed) && (len & (len - 1)))
        return fail(GMSM_ERR_ARG, std::string(E) + ": len must be a power of 2 in a Lagrange basis or a BitReverse layout");
    if (basis != 1 && len > ((size_t)1 << vt->fr_max_order)) return fail(GMSM_ERR_ARG, ERR_ROOT);
    if (shift && size > ((size_t)1 << vt->fr_max_order)) return fail(GMSM_ERR_ARG, ERR_ROOT);  // fft.Generator(size)
    if (k > (((size_t)1 << 62) / len)) return fail(GMSM_ERR_ARG, std::string(E) + ": k * len does not fit");
    if (polys && ratio_overlap(out_values, nullptr, k * vt->scalar_bytes, polys, nullptr, k * len * vt->scalar_bytes)) return ratio_aliases(E);
    Context *ctx;
    if ((rc = enter_owner(d_polys, &ctx))) return rc;
    if ((rc = check_device_vector(E, "d_polys", d_polys, ctx->device))) return rc;
    return vt->iop_evaluate(*ctx, polys, d_polys, k, len, size, basis, layouts, shift, coset, x, (hipStream_t)hip_stream, out_values);
}

GMSM_EXPORT int gmsm_iop_divide_by_x_minus_one(uint64_t domain_small, uint64_t domain_big, const uint64_t *a, const void *d_a, int basis,
                                               int layout, uint64_t shift, void *hip_stream, uint64_t *out, void *d_out) {
    const char *E = "gmsm_iop_divide_by_x_minus_one";
    int rc = ratio_pair(E, "a", "d_a", a, d_a);
    if (rc || (rc = ratio_pair(E, "out", "d_out", out, d_out)) || (rc = iop_basis(E, "basis", basis))) return rc;
    if (basis != 4) return fail(GMSM_ERR_ARG, "the basis must be LagrangeCoset");  // ErrMustBeLagrangeCoset
    if ((rc = iop_layout(E, layout))) return rc;
    FftRef small = g_fft.get(domain_small), big = g_fft.get(domain_big);
    if (!small || !big) return fail(GMSM_ERR_ARG, "unknown fft domain handle");
    if ((small->group & ~1) != (big->group & ~1)) return fail(GMSM_ERR_ARG, std::string(E) + ": the two domains are of different curves");
    if (small->log2n > big->log2n) return fail(GMSM_ERR_ARG, std::string(E) + ": the small domain is larger than the big one");
    const FieldVTable *vt = fr_vtable(big->group);
    const size_t bytes = vt->scalar_bytes << big->log2n;
    if (ratio_overlap(out, d_out, bytes, a, d_a, bytes)) return ratio_aliases(E);
    Context *ctx;
    if ((rc = enter_on(big->device, &ctx))) return rc;  // the big domain decides the device
    if ((rc = check_device_vector(E, "d_a", d_a, ctx->device)) || (rc = check_device_vector(E, "d_out", d_out, ctx->device))) return rc;
    return vt->iop_quotient(*ctx, small.get(), big.get(), a, d_a, layout, (size_t)(shift & (((uint64_t)1 << small->log2n) - 1)),
                            (hipStream_t)hip_stream, out, d_out);
}

// ------------------------------------------------------------------ iop.Evaluate of a straight-line program (gmsm_iop_expr.h)
// The program's checks, in instruction order, so that the kernel never sees a bad one: every text names the instruction.
// *nregs = the registers the program uses (a read is of a register written before, so the writes bound them).
static int expr_validate(const char *E, const uint32_t *prog, size_t prog_len, size_t m, size_t n_consts, bool has_domain, unsigned *nregs,
                         bool *has_point) {
    if (prog_len == 0) return fail(GMSM_ERR_ARG, std::string(E) + ": empty program");
    if (prog_len > GMSM_EXPR_MAX_INSNS)
        return fail(GMSM_ERR_ARG, std::string(E) + ": the program has " + std::to_string(prog_len) + " instructions, more than " +
                                      std::to_string(GMSM_EXPR_MAX_INSNS));
    uint32_t written = 0;
    *nregs = 0, *has_point = false;
    for (size_t pc = 0; pc < prog_len; ++pc) {
        const uint32_t ins = prog[pc];
        const unsigned op = ins & 0xff, dst = (ins >> 8) & 0xff, a = (ins >> 16) & 0xff, b = ins >> 24;
        const std::string at = std::string(E) + ": instruction " + std::to_string(pc) + ": ";
        auto reads = [&](unsigned reg) {
            if (reg >= GMSM_EXPR_MAX_REGS) return fail(GMSM_ERR_ARG, at + "register " + std::to_string(reg) + " is not below " + std::to_string(GMSM_EXPR_MAX_REGS));
            if (!((written >> reg) & 1)) return fail(GMSM_ERR_ARG, at + "reads register " + std::to_string(reg) + " before any instruction wrote it");
            return (int)GMSM_OK;
        };
        int rc = GMSM_OK;
        switch (op) {
            case GMSM_EXPR_INPUT:
                if (a >= m) return fail(GMSM_ERR_ARG, at + "input " + std::to_string(a) + " of " + std::to_string(m));
                break;
            case GMSM_EXPR_CONST:
                if (a >= n_consts) return fail(GMSM_ERR_ARG, at + "constant " + std::to_string(a) + " of " + std::to_string(n_consts));
                break;
            case GMSM_EXPR_POINT:
                if (!has_domain) return fail(GMSM_ERR_ARG, at + "POINT needs a domain (domain == 0)");
                *has_point = true;
                break;
            case GMSM_EXPR_ADD:
            case GMSM_EXPR_SUB:
            case GMSM_EXPR_MUL:
                if ((rc = reads(a)) || (rc = reads(b))) return rc;
                break;
            case GMSM_EXPR_NEG:
                if ((rc = reads(a))) return rc;
                break;
            default: return fail(GMSM_ERR_ARG, at + "unknown opcode " + std::to_string(op));
        }
        if (dst >= GMSM_EXPR_MAX_REGS) return fail(GMSM_ERR_ARG, at + "register " + std::to_string(dst) + " is not below " + std::to_string(GMSM_EXPR_MAX_REGS));
        written |= 1u << dst;
        *nregs = std::max(*nregs, dst + 1);
    }
    return GMSM_OK;
}

GMSM_EXPORT int gmsm_iop_evaluate_expression(int group, uint64_t domain, const uint32_t *prog, size_t prog_len, const uint64_t *consts,
                                             size_t n_consts, const uint64_t *const *polys, const void *const *d_polys, size_t m, size_t len,
                                             const size_t *sizes, const int64_t *shifts, const uint32_t *layouts, int out_layout, void *hip_stream,
                                             uint64_t *out, void *d_out) {
    FR_OR_FAIL(group);
    const char *E = "gmsm_iop_evaluate_expression";
    if (len == 0) return GMSM_OK;
    if (m == 0) return fail(GMSM_ERR_ARG, std::string(E) + ": need at least one input (m == 0)");
    if (m > GMSM_EXPR_MAX_INPUTS) return fail(GMSM_ERR_ARG, std::string(E) + ": " + std::to_string(m) + " inputs, more than " + std::to_string(GMSM_EXPR_MAX_INPUTS));
    if (n_consts > GMSM_EXPR_MAX_CONSTS)
        return fail(GMSM_ERR_ARG, std::string(E) + ": " + std::to_string(n_consts) + " constants, more than " + std::to_string(GMSM_EXPR_MAX_CONSTS));
    if (!prog) return fail(GMSM_ERR_ARG, std::string(E) + ": prog is null");
    if (n_consts && !consts) return fail(GMSM_ERR_ARG, std::string(E) + ": consts is null");
    if (!sizes || !shifts) return fail(GMSM_ERR_ARG, std::string(E) + ": sizes and shifts must not be null");
    int rc = ratio_layouts(E, "layouts", layouts, m);
    if (rc || (rc = iop_layout(E, out_layout)) || (rc = ratio_pair(E, "polys", "d_polys", polys, d_polys)) ||
        (rc = ratio_pair(E, "out", "d_out", out, d_out)))
        return rc;
    const void *const *in = polys ? (const void *const *)polys : d_polys;
    for (size_t j = 0; j < m; ++j)
        if (!in[j]) return fail(GMSM_ERR_ARG, std::string(E) + ": " + (polys ? "polys[" : "d_polys[") + std::to_string(j) + "] is null");
    unsigned nregs = 0;
    bool has_point = false, reversed = out_layout == 16;
    if ((rc = expr_validate(E, prog, prog_len, m, n_consts, domain != 0, &nregs, &has_point))) return rc;
    std::vector<size_t> offsets(m);
    for (size_t j = 0; j < m; ++j) {
        reversed = reversed || layouts[j] == 16;
        if (sizes[j] == 0 || sizes[j] > len)
            return fail(GMSM_ERR_ARG, std::string(E) + ": sizes[" + std::to_string(j) + "] = " + std::to_string(sizes[j]) + " is outside [1, len]");
        if (shifts[j] < 0)
            return fail(GMSM_ERR_ARG, std::string(E) + ": shifts[" + std::to_string(j) + "] = " + std::to_string(shifts[j]) +
                                          " is negative (the reference panics on the index)");
        // rho shift mod len without overflow: both factors are reduced first, and their product is below len^2
        const size_t rho = len / sizes[j];
        offsets[j] = (size_t)(((unsigned __int128)(rho % len) * ((uint64_t)shifts[j] % len)) % len);
    }
    if ((reversed || has_point) && (len & (len - 1)))
        return fail(GMSM_ERR_ARG, std::string(E) + ": len must be a power of 2 with a BitReverse layout or a POINT instruction");
    if (len > ((size_t)1 << 62) / (m * vt->scalar_bytes)) return fail(GMSM_ERR_ARG, std::string(E) + ": m * len does not fit");
    FftRef d;
    if (domain != 0) {
        if (!(d = g_fft.get(domain))) return fail(GMSM_ERR_ARG, "unknown fft domain handle");
        if ((d->group & ~1) != (group & ~1)) return fail(GMSM_ERR_ARG, std::string(E) + ": the domain is of another curve");
        if (has_point && ((size_t)1 << d->log2n) != len)
            return fail(GMSM_ERR_ARG, std::string(E) + ": the domain's cardinality " + std::to_string((size_t)1 << d->log2n) + " is not len " +
                                          std::to_string(len) + " (POINT is w^i with w = fft.Generator(len))");
    }
    // The output may be input j itself when the lane that reads a slot is the lane that writes it; any other shared byte is refused
    const size_t bytes = len * vt->scalar_bytes;
    const uintptr_t o = (uintptr_t)(out ? (const void *)out : (const void *)d_out);
    for (size_t j = 0; j < m; ++j) {
        const uintptr_t i = (uintptr_t)in[j];
        if ((out != nullptr) != (polys != nullptr) || !(o < i + bytes && i < o + bytes)) continue;
        if (o != i) return ratio_aliases(E);
        if (layouts[j] != (uint32_t)out_layout || offsets[j] != 0)
            return fail(GMSM_ERR_ARG, std::string(E) + ": the output is input " + std::to_string(j) +
                                          ", which needs the same layout and no offset (the lane that reads a slot must be the one that writes it)");
    }
    Context *ctx;
    if (d && has_point) rc = enter_on(d->device, &ctx);  // the domain decides the device
    else rc = enter_owner(d_polys ? d_polys[0] : d_out, &ctx);
    if (rc) return rc;
    if (d_polys)
        for (size_t j = 0; j < m; ++j)
            if ((rc = check_device_vector(E, ("d_polys[" + std::to_string(j) + "]").c_str(), d_polys[j], ctx->device))) return rc;
    if ((rc = check_device_vector(E, "d_out", d_out, ctx->device))) return rc;
    return vt->iop_expr(*ctx, has_point ? d.get() : nullptr, prog, prog_len, nregs, consts, n_consts, polys, d_polys, m, len, offsets.data(), layouts,
                        out_layout, (hipStream_t)hip_stream, out, d_out);
}

// ------------------------------------------------------------------ fr/polynomial.MultiLin and one GKR sumcheck claim (gmsm_gkr.h)
using GkrRef = std::shared_ptr<GkrClaim>;
static HandleTable<GkrClaim> g_gkr;

// len = 2^*n, or the refusal
static int multilin_len(const char *E, size_t len, size_t scalar_bytes, unsigned *n) {
    if (len == 0 || (len & (len - 1)))
        return fail(GMSM_ERR_ARG, std::string(E) + ": len = " + std::to_string(len) + " is not a power of two (a MultiLin has 2^n elements)");
    if (len > ((size_t)1 << 62) / scalar_bytes) return fail(GMSM_ERR_ARG, std::string(E) + ": len does not fit");
    for (*n = 0; ((size_t)1 << *n) < len; ++*n) {
    }
    return GMSM_OK;
}

GMSM_EXPORT int gmsm_multilin_fold(int group, uint64_t *a, void *d_a, size_t len, const uint64_t *r, void *hip_stream) {
    FR_OR_FAIL(group);
    const char *E = "gmsm_multilin_fold";
    unsigned n;
    int rc = multilin_len(E, len, vt->scalar_bytes, &n);
    if (rc) return rc;
    if (len == 1) return fail(GMSM_ERR_ARG, std::string(E) + ": len == 1: nothing to fold");
    if (!r) return fail(GMSM_ERR_ARG, std::string(E) + ": r is null");
    if ((rc = ratio_pair(E, "a", "d_a", a, d_a))) return rc;
    Context *ctx;
    if ((rc = enter_owner(d_a, &ctx)) || (rc = check_device_vector(E, "d_a", d_a, ctx->device))) return rc;
    return vt->multilin_fold(*ctx, a, d_a, len, r, (hipStream_t)hip_stream);
}

GMSM_EXPORT int gmsm_multilin_evaluate(int group, const uint64_t *m, const void *d_m, size_t len, const uint64_t *coords, size_t ncoords,
                                       void *hip_stream, uint64_t *out_value) {
    FR_OR_FAIL(group);
    const char *E = "gmsm_multilin_evaluate";
    unsigned n;
    int rc = multilin_len(E, len, vt->scalar_bytes, &n);
    if (rc) return rc;
    if (ncoords > n)
        return fail(GMSM_ERR_ARG, std::string(E) + ": ncoords = " + std::to_string(ncoords) + " is more than log2 len = " + std::to_string(n));
    if (ncoords && !coords) return fail(GMSM_ERR_ARG, std::string(E) + ": coords is null");
    if (!out_value) return fail(GMSM_ERR_ARG, std::string(E) + ": out_value is null");
    if ((rc = ratio_pair(E, "m", "d_m", m, d_m))) return rc;
    Context *ctx;
    if ((rc = enter_owner(d_m, &ctx)) || (rc = check_device_vector(E, "d_m", d_m, ctx->device))) return rc;
    return vt->multilin_evaluate(*ctx, m, d_m, len, coords, ncoords, (hipStream_t)hip_stream, out_value);
}

GMSM_EXPORT int gmsm_multilin_eq(int group, const uint64_t *q, size_t n, const uint64_t *scale, int accumulate, void *hip_stream, uint64_t *out,
                                 void *d_out) {
    FR_OR_FAIL(group);
    const char *E = "gmsm_multilin_eq";
    if (n >= 8 * sizeof(size_t) || ((size_t)1 << n) > ((size_t)1 << 62) / vt->scalar_bytes)
        return fail(GMSM_ERR_ARG, std::string(E) + ": n = " + std::to_string(n) + ": 2^n elements are beyond what size_t indexes");
    if (n && !q) return fail(GMSM_ERR_ARG, std::string(E) + ": q is null");
    if (!scale) return fail(GMSM_ERR_ARG, std::string(E) + ": scale is null");
    int rc = ratio_pair(E, "out", "d_out", out, d_out);
    if (rc) return rc;
    if (out && n) {
        const uintptr_t o = (uintptr_t)out, ob = ((size_t)1 << n) * vt->scalar_bytes, p = (uintptr_t)q, pb = n * vt->scalar_bytes;
        if (o < p + pb && p < o + ob) return fail(GMSM_ERR_ARG, std::string(E) + ": out overlaps q");
    }
    Context *ctx;
    if ((rc = enter_owner(d_out, &ctx)) || (rc = check_device_vector(E, "d_out", d_out, ctx->device))) return rc;
    return vt->multilin_eq(*ctx, q, (unsigned)n, scale, accumulate, (hipStream_t)hip_stream, out, d_out);
}

GMSM_EXPORT int gmsm_gkr_claim_new(int group, const uint32_t *prog, size_t prog_len, const uint64_t *consts, size_t n_consts, size_t degree,
                                   const uint64_t *const *tables, const void *const *d_tables, size_t m, size_t len, const uint64_t *points, size_t k,
                                   const uint64_t *comb, void *hip_stream, uint64_t *out_gj, uint64_t *out_handle) {
    FR_OR_FAIL(group);
    const char *E = "gmsm_gkr_claim_new";
    unsigned n;
    int rc = multilin_len(E, len, vt->scalar_bytes, &n);
    if (rc) return rc;
    if (len == 1) return fail(GMSM_ERR_ARG, std::string(E) + ": len == 1: a sumcheck needs at least one variable");
    if (m == 0) return fail(GMSM_ERR_ARG, std::string(E) + ": need at least one input (m == 0)");
    if (m > GMSM_GKR_MAX_INPUTS) return fail(GMSM_ERR_ARG, std::string(E) + ": " + std::to_string(m) + " inputs, more than " + std::to_string(GMSM_GKR_MAX_INPUTS));
    if (degree == 0 || degree > GMSM_GKR_MAX_DEGREE)
        return fail(GMSM_ERR_ARG, std::string(E) + ": degree = " + std::to_string(degree) + " is outside [1, " + std::to_string(GMSM_GKR_MAX_DEGREE) + "]");
    if (k == 0) return fail(GMSM_ERR_ARG, std::string(E) + ": need at least one evaluation point (k == 0)");
    if (k >= 2 && !comb) return fail(GMSM_ERR_ARG, std::string(E) + ": comb is null with k >= 2");
    if (n_consts > GMSM_EXPR_MAX_CONSTS)
        return fail(GMSM_ERR_ARG, std::string(E) + ": " + std::to_string(n_consts) + " constants, more than " + std::to_string(GMSM_EXPR_MAX_CONSTS));
    if (!prog) return fail(GMSM_ERR_ARG, std::string(E) + ": prog is null");
    if (n_consts && !consts) return fail(GMSM_ERR_ARG, std::string(E) + ": consts is null");
    if (!points) return fail(GMSM_ERR_ARG, std::string(E) + ": points is null");
    if (!out_gj || !out_handle) return fail(GMSM_ERR_ARG, std::string(E) + ": out_gj and out_handle must not be null");
    if ((rc = ratio_pair(E, "tables", "d_tables", tables, d_tables))) return rc;
    const void *const *in = tables ? (const void *const *)tables : d_tables;
    for (size_t j = 0; j < m; ++j)
        if (!in[j]) return fail(GMSM_ERR_ARG, std::string(E) + ": " + (tables ? "tables[" : "d_tables[") + std::to_string(j) + "] is null");
    unsigned nregs = 0;
    bool has_point = false;
    if ((rc = expr_validate(E, prog, prog_len, m, n_consts, false, &nregs, &has_point))) return rc;  // POINT: a gate has no index
    if (len > ((size_t)1 << 62) / ((m + 1) * vt->scalar_bytes) || k > ((size_t)1 << 40))
        return fail(GMSM_ERR_ARG, std::string(E) + ": (m + 1) * len or k does not fit");
    Context *ctx;
    if ((rc = enter_owner(d_tables ? d_tables[0] : nullptr, &ctx))) return rc;
    if (d_tables)
        for (size_t j = 0; j < m; ++j)
            if ((rc = check_device_vector(E, ("d_tables[" + std::to_string(j) + "]").c_str(), d_tables[j], ctx->device))) return rc;
    GkrRef c = std::make_shared<GkrClaim>();
    c->group = group & ~1, c->device = ctx->device, c->stream = (hipStream_t)hip_stream;
    c->m = m, c->degree = degree, c->stride = c->len = len, c->nregs = nregs, c->prog_len = (uint32_t)prog_len;
    if ((rc = vt->gkr_new(*ctx, c.get(), prog, consts, n_consts, tables, d_tables, points, k, comb, out_gj))) return rc;
    *out_handle = g_gkr.add(c);
    return GMSM_OK;
}

// The claim of a handle, locked for one call; refuses an unknown handle and a finished claim
static int gkr_claim(const char *E, uint64_t handle, const void *r, const void *out, GkrRef *c, const FieldVTable **vt) {
    if (!(*c = g_gkr.get(handle))) return fail(GMSM_ERR_ARG, "unknown gkr claim handle");
    if (!r || !out) return fail(GMSM_ERR_ARG, std::string(E) + ": r and the output must not be null");
    *vt = fr_vtable((*c)->group);
    return GMSM_OK;
}

GMSM_EXPORT int gmsm_gkr_claim_next(uint64_t handle, const uint64_t *r, uint64_t *out_gj) {
    const char *E = "gmsm_gkr_claim_next";
    GkrRef c;
    const FieldVTable *vt;
    int rc = gkr_claim(E, handle, r, out_gj, &c, &vt);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->finished) return fail(GMSM_ERR_ARG, "the claim is finished");
    if (c->len == 2)
        return fail(GMSM_ERR_ARG, std::string(E) + ": the tables have length 2: no variable is left for a round (call gmsm_gkr_claim_final)");
    Context *ctx;
    if ((rc = enter_on(c->device, &ctx))) return rc;
    if ((rc = vt->gkr_next(c.get(), r, out_gj))) c->finished = true;  // a device error: the tables may be half folded
    return rc;
}

GMSM_EXPORT int gmsm_gkr_claim_final(uint64_t handle, const uint64_t *r, uint64_t *out_evals) {
    const char *E = "gmsm_gkr_claim_final";
    GkrRef c;
    const FieldVTable *vt;
    int rc = gkr_claim(E, handle, r, out_evals, &c, &vt);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->finished) return fail(GMSM_ERR_ARG, "the claim is finished");
    if (c->len != 2)
        return fail(GMSM_ERR_ARG, std::string(E) + ": the tables have length " + std::to_string(c->len) + ", not 2 (call gmsm_gkr_claim_next)");
    Context *ctx;
    if ((rc = enter_on(c->device, &ctx))) return rc;
    c->finished = true;
    return vt->gkr_final(c.get(), r, out_evals);
}

GMSM_EXPORT int gmsm_gkr_claim_release(uint64_t handle) {
    if (!g_gkr.take(handle)) return fail(GMSM_ERR_ARG, "unknown gkr claim handle");  // the tables go with the last reference
    return GMSM_OK;
}

// ------------------------------------------------------------------ fr/mimc and the Merkle tree over it (gmsm_mimc.h)
using MerkleRef = std::shared_ptr<MerkleTree>;
static HandleTable<MerkleTree> g_merkle;

GMSM_EXPORT int gmsm_mimc_constants(int group, uint64_t *out, unsigned *out_rounds) {
    FR_OR_FAIL(group);
    if (!out && !out_rounds) return fail(GMSM_ERR_ARG, "gmsm_mimc_constants: out and out_rounds are both null");
    if (out) vt->mimc_constants(out);
    if (out_rounds) *out_rounds = vt->mimc_rounds;
    return GMSM_OK;
}

GMSM_EXPORT int gmsm_mimc_hash(int group, const uint64_t *state, const uint64_t *elems, size_t len, uint64_t *out) {
    FR_OR_FAIL(group);
    const char *E = "gmsm_mimc_hash";
    if (!out) return fail(GMSM_ERR_ARG, std::string(E) + ": out is null");
    if (len && !elems) return fail(GMSM_ERR_ARG, std::string(E) + ": elems is null");
    vt->mimc_hash(state, elems, len, out);
    return GMSM_OK;
}

GMSM_EXPORT int gmsm_mimc_sum_batch(int group, const uint64_t *msgs, const void *d_msgs, size_t count, size_t len, size_t stride, const uint64_t *state,
                                    void *hip_stream, uint64_t *out, void *d_out) {
    FR_OR_FAIL(group);
    const char *E = "gmsm_mimc_sum_batch";
    if (count == 0) return GMSM_OK;
    if (stride < len) return fail(GMSM_ERR_ARG, std::string(E) + ": stride = " + std::to_string(stride) + " is less than len = " + std::to_string(len));
    int rc;
    if (len) {
        if ((rc = ratio_pair(E, "msgs", "d_msgs", msgs, d_msgs))) return rc;
    } else if (msgs && d_msgs) {  // nothing is read: none is fine, two is a mistake
        return fail(GMSM_ERR_ARG, std::string(E) + ": give at most one of msgs (host) / d_msgs (device)");
    }
    if ((rc = ratio_pair(E, "out", "d_out", out, d_out))) return rc;
    const size_t limit = ((size_t)1 << 62) / vt->scalar_bytes;
    if (count > limit || (len && stride > limit / count)) return fail(GMSM_ERR_ARG, std::string(E) + ": count * stride does not fit");
    const size_t in_bytes = len ? ((count - 1) * stride + len) * vt->scalar_bytes : 0, out_bytes = count * vt->scalar_bytes;
    if (in_bytes && ratio_overlap(out, d_out, out_bytes, msgs, d_msgs, in_bytes)) return ratio_aliases(E);
    if (out && !len) {  // count copies of the state: no device work
        for (size_t i = 0; i < count; ++i) vt->mimc_hash(state, nullptr, 0, out + i * (vt->scalar_bytes / 8));
        return GMSM_OK;
    }
    Context *ctx;
    if ((rc = enter_owner(d_msgs ? d_msgs : d_out, &ctx))) return rc;
    if ((rc = check_device_vector(E, "d_msgs", d_msgs, ctx->device)) || (rc = check_device_vector(E, "d_out", d_out, ctx->device))) return rc;
    return vt->mimc_sum_batch(*ctx, msgs, len ? d_msgs : nullptr, count, len, stride, state, (hipStream_t)hip_stream, out, d_out);
}

GMSM_EXPORT int gmsm_merkle_new(int group, const uint64_t *leaves, const void *d_leaves, size_t n, size_t leaf_len, int keep_leaves, void *hip_stream,
                                uint64_t *out_handle) {
    FR_OR_FAIL(group);
    const char *E = "gmsm_merkle_new";
    if (n == 0) return fail(GMSM_ERR_ARG, std::string(E) + ": no leaf (n == 0)");
    if (leaf_len == 0) return fail(GMSM_ERR_ARG, std::string(E) + ": empty leaves (leaf_len == 0)");
    if (!out_handle) return fail(GMSM_ERR_ARG, std::string(E) + ": out_handle is null");
    int rc = ratio_pair(E, "leaves", "d_leaves", leaves, d_leaves);
    if (rc) return rc;
    const size_t limit = ((size_t)1 << 61) / vt->scalar_bytes;
    if (n > limit || leaf_len > limit / n) return fail(GMSM_ERR_ARG, std::string(E) + ": n * leaf_len does not fit");
    Context *ctx;
    if ((rc = enter_owner(d_leaves, &ctx)) || (rc = check_device_vector(E, "d_leaves", d_leaves, ctx->device))) return rc;
    MerkleRef t = std::make_shared<MerkleTree>();
    t->group = group & ~1, t->device = ctx->device, t->n = n, t->leaf_len = leaf_len;
    for (size_t size = n;; size = (size + 1) / 2) {
        t->total += size;
        if (size == 1) break;
        ++t->depth;
    }
    if ((rc = vt->merkle_new(*ctx, t.get(), leaves, d_leaves, keep_leaves != 0, (hipStream_t)hip_stream))) return rc;
    *out_handle = g_merkle.add(t);
    return GMSM_OK;
}

GMSM_EXPORT int gmsm_merkle_info(uint64_t handle, size_t *out_n, size_t *out_leaf_len, unsigned *out_depth) {
    MerkleRef t = g_merkle.get(handle);
    if (!t) return fail(GMSM_ERR_ARG, "unknown merkle tree handle");
    if (out_n) *out_n = t->n;
    if (out_leaf_len) *out_leaf_len = t->leaf_len;
    if (out_depth) *out_depth = t->depth;
    return GMSM_OK;
}

GMSM_EXPORT int gmsm_merkle_root(uint64_t handle, uint64_t *out_root) {
    MerkleRef t = g_merkle.get(handle);
    if (!t) return fail(GMSM_ERR_ARG, "unknown merkle tree handle");
    if (!out_root) return fail(GMSM_ERR_ARG, "gmsm_merkle_root: out_root is null");
    memcpy(out_root, t->root.data(), t->root.size() * sizeof(uint64_t));
    return GMSM_OK;
}

GMSM_EXPORT int gmsm_merkle_prove(uint64_t handle, const uint64_t *indices, size_t k, uint64_t *out_leaves, uint64_t *out_siblings,
                                  uint32_t *out_counts) {
    const char *E = "gmsm_merkle_prove";
    MerkleRef t = g_merkle.get(handle);
    if (!t) return fail(GMSM_ERR_ARG, "unknown merkle tree handle");
    if (k == 0) return GMSM_OK;
    if (!indices || !out_counts || (t->depth && !out_siblings))
        return fail(GMSM_ERR_ARG, std::string(E) + ": indices, out_siblings and out_counts must not be null");
    if (out_leaves && !t->leaves.ptr) return fail(GMSM_ERR_ARG, std::string(E) + ": out_leaves is given, but the tree was built without keep_leaves");
    const FieldVTable *vt = fr_vtable(t->group);
    if (k > ((size_t)1 << 61) / (vt->scalar_bytes * (t->depth + t->leaf_len))) return fail(GMSM_ERR_ARG, std::string(E) + ": k does not fit");
    for (size_t j = 0; j < k; ++j)
        if (indices[j] >= t->n)
            return fail(GMSM_ERR_ARG, std::string(E) + ": indices[" + std::to_string(j) + "] = " + std::to_string(indices[j]) + " is outside [0, " +
                                          std::to_string(t->n) + ")");
    Context *ctx;
    if (int rc = enter_on(t->device, &ctx)) return rc;
    return vt->merkle_prove(*ctx, t.get(), indices, k, out_leaves, out_siblings, out_counts);
}

GMSM_EXPORT int gmsm_merkle_release(uint64_t handle) {
    if (!g_merkle.take(handle)) return fail(GMSM_ERR_ARG, "unknown merkle tree handle");  // the levels go with the last reference
    return GMSM_OK;
}

// ------------------------------------------------------------------ fr/fri's prover (gmsm_fri.h)
using FriRef = std::shared_ptr<FriOracle>;
static HandleTable<FriOracle> g_fri;

GMSM_EXPORT int gmsm_fri_commit(uint64_t domain, const uint64_t *p, const void *d_p, size_t len, void *hip_stream, uint64_t *out_oracle) {
    const char *E = "gmsm_fri_commit";
    FftRef d = g_fft.get(domain);
    if (!d) return fail(GMSM_ERR_ARG, "unknown fft domain handle");
    const FieldVTable *vt = fr_vtable(d->group);
    const size_t N = (size_t)1 << d->log2n;
    if (d->log2n < 4)
        return fail(GMSM_ERR_ARG, std::string(E) + ": the domain's cardinality " + std::to_string(N) + " is below 16 (rho = 8 times a size of at least 2)");
    if (len > N) return fail(GMSM_ERR_ARG, std::string(E) + ": len = " + std::to_string(len) + " is more than the domain's cardinality " + std::to_string(N));
    if (!out_oracle) return fail(GMSM_ERR_ARG, std::string(E) + ": out_oracle is null");
    int rc = ratio_pair(E, "p", "d_p", p, d_p);
    if (rc) return rc;
    Context *ctx;
    if ((rc = enter_on(d->device, &ctx)) || (rc = check_device_vector(E, "d_p", d_p, ctx->device))) return rc;
    FriRef o = std::make_shared<FriOracle>();
    o->group = d->group & ~1, o->device = d->device, o->log2n = d->log2n, o->nb_steps = d->log2n - 3, o->domain = d;
    if ((rc = vt->fri_commit(*ctx, o.get(), p, d_p, len, (hipStream_t)hip_stream))) return rc;
    *out_oracle = g_fri.add(o);
    return GMSM_OK;
}

GMSM_EXPORT int gmsm_fri_info(uint64_t oracle, uint64_t *out_cardinality, unsigned *out_nb_steps, unsigned *out_folds_done) {
    FriRef o = g_fri.get(oracle);
    if (!o) return fail(GMSM_ERR_ARG, "unknown fri oracle handle");
    std::lock_guard<std::mutex> lk(o->mu);
    if (out_cardinality) *out_cardinality = (uint64_t)1 << o->log2n;
    if (out_nb_steps) *out_nb_steps = o->nb_steps;
    if (out_folds_done) *out_folds_done = o->folds_done;
    return GMSM_OK;
}

// refuses a step whose layer is not built; the caller holds the oracle's lock
static int fri_step(const char *E, const FriOracle &o, size_t step) {
    if (step < o.trees.size()) return GMSM_OK;
    return fail(GMSM_ERR_ARG, std::string(E) + ": step " + std::to_string(step) + " is not built (" + std::to_string(o.trees.size()) + " of " +
                                  std::to_string(o.nb_steps) + " layers are)");
}

GMSM_EXPORT int gmsm_fri_root(uint64_t oracle, unsigned step, uint64_t *out_root) {
    const char *E = "gmsm_fri_root";
    FriRef o = g_fri.get(oracle);
    if (!o) return fail(GMSM_ERR_ARG, "unknown fri oracle handle");
    if (!out_root) return fail(GMSM_ERR_ARG, std::string(E) + ": out_root is null");
    std::lock_guard<std::mutex> lk(o->mu);
    if (int rc = fri_step(E, *o, step)) return rc;
    const std::vector<uint64_t> &root = o->trees[step]->root;
    memcpy(out_root, root.data(), root.size() * sizeof(uint64_t));
    return GMSM_OK;
}

GMSM_EXPORT int gmsm_fri_fold(uint64_t oracle, const uint64_t *xi, uint64_t *out) {
    const char *E = "gmsm_fri_fold";
    FriRef o = g_fri.get(oracle);
    if (!o) return fail(GMSM_ERR_ARG, "unknown fri oracle handle");
    if (!xi || !out) return fail(GMSM_ERR_ARG, std::string(E) + ": xi and out must not be null");
    std::lock_guard<std::mutex> lk(o->mu);
    if (o->folds_done >= o->nb_steps)
        return fail(GMSM_ERR_ARG, std::string(E) + ": all " + std::to_string(o->nb_steps) + " folds are done");
    Context *ctx;
    if (int rc = enter_on(o->device, &ctx)) return rc;
    return fr_vtable(o->group)->fri_fold(*ctx, o.get(), xi, out);
}

GMSM_EXPORT int gmsm_fri_layer(uint64_t oracle, unsigned step, uint64_t *out, void *d_out) {
    const char *E = "gmsm_fri_layer";
    FriRef o = g_fri.get(oracle);
    if (!o) return fail(GMSM_ERR_ARG, "unknown fri oracle handle");
    int rc = ratio_pair(E, "out", "d_out", out, d_out);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(o->mu);
    if ((rc = fri_step(E, *o, step))) return rc;
    Context *ctx;
    if ((rc = enter_on(o->device, &ctx)) || (rc = check_device_vector(E, "d_out", d_out, ctx->device))) return rc;
    return fr_vtable(o->group)->fri_layer(*ctx, o.get(), step, out, d_out);
}

GMSM_EXPORT int gmsm_fri_query(uint64_t oracle, const uint64_t *positions, size_t count, uint64_t *out_pairs, uint64_t *out_leaf_sums,
                               uint64_t *out_siblings, uint32_t *out_counts) {
    const char *E = "gmsm_fri_query";
    FriRef o = g_fri.get(oracle);
    if (!o) return fail(GMSM_ERR_ARG, "unknown fri oracle handle");
    if (count == 0) return GMSM_OK;
    if (!positions || !out_pairs || !out_leaf_sums || !out_siblings || !out_counts)
        return fail(GMSM_ERR_ARG, std::string(E) + ": positions and the four outputs must not be null");
    std::lock_guard<std::mutex> lk(o->mu);
    int rc = fri_step(E, *o, count - 1);
    if (rc) return rc;
    for (size_t i = 0; i < count; ++i)
        if (positions[i] >= o->trees[i]->n)
            return fail(GMSM_ERR_ARG, std::string(E) + ": positions[" + std::to_string(i) + "] = " + std::to_string(positions[i]) + " is outside [0, " +
                                          std::to_string(o->trees[i]->n) + ")");
    Context *ctx;
    if ((rc = enter_on(o->device, &ctx))) return rc;
    return fr_vtable(o->group)->fri_query(*ctx, o.get(), positions, count, out_pairs, out_leaf_sums, out_siblings, out_counts);
}

GMSM_EXPORT int gmsm_fri_release(uint64_t oracle) {
    if (!g_fri.take(oracle)) return fail(GMSM_ERR_ARG, "unknown fri oracle handle");  // the layers go with the last reference
    return GMSM_OK;
}

// ------------------------------------------------------------------ fixed-base batch
GMSM_EXPORT int gmsm_batch_scalar_mul(int group, const uint64_t *base_affine, const uint64_t *scalars, size_t n,
                                      uint64_t *out_affine) {
    VT_OR_FAIL(group);
    if (!base_affine || (n && (!scalars || !out_affine))) return fail(GMSM_ERR_ARG, "gmsm_batch_scalar_mul: null argument");
    Context *ctx;
    int rc = enter(&ctx);
    if (rc) return rc;
    return vt->batch_scalar_mul(*ctx, base_affine, scalars, nullptr, n, nullptr, out_affine, nullptr);
}

GMSM_EXPORT int gmsm_batch_scalar_mul_device(int group, const uint64_t *base_affine, const void *d_scalars, size_t n,
                                             void *hip_stream, void *d_out_affine) {
    VT_OR_FAIL(group);
    if (!base_affine || (n && (!d_scalars || !d_out_affine)))
        return fail(GMSM_ERR_ARG, "gmsm_batch_scalar_mul_device: null argument");
    Context *ctx;
    int rc = enter_owner(d_scalars, &ctx);
    if (rc) return rc;
    return vt->batch_scalar_mul(*ctx, base_affine, nullptr, d_scalars, n, (hipStream_t)hip_stream, nullptr, d_out_affine);
}

GMSM_EXPORT int gmsm_batch_jac_to_affine(int group, const uint64_t *jac, size_t n, uint64_t *out_affine) {
    VT_OR_FAIL(group);
    if (n && (!jac || !out_affine)) return fail(GMSM_ERR_ARG, "gmsm_batch_jac_to_affine: null argument");
    Context *ctx;
    int rc = enter(&ctx);
    if (rc) return rc;
    return vt->batch_jac_to_affine(*ctx, jac, n, out_affine);
}

GMSM_EXPORT unsigned gmsm_default_window_bits(int group, size_t n) {
    const GroupVTable *vt = vtable(group);
    return vt ? choose_c(vt->fr_bits, vt->aff_bytes, n) : 0;
}

GMSM_EXPORT int gmsm_default_plan(int group, size_t n, unsigned *c, unsigned *nwin, unsigned *entries_per_point, unsigned *fused) {
    VT_OR_FAIL(group);
    unsigned a = 0, b = 0, e = 1, f = 0;
    vt->plan_info(n, &a, &b, &e, &f);
    if (c) *c = a;
    if (nwin) *nwin = b;
    if (entries_per_point) *entries_per_point = e;
    if (fused) *fused = f;
    return GMSM_OK;
}

GMSM_EXPORT int gmsm_debug_reduce_shape(int group, uint32_t nw, uint32_t nbuckets, uint32_t out[6]) {
    VT_OR_FAIL(group);
    if (nw == 0 || nbuckets == 0 || nbuckets > (1u << 19) || !out) return fail(GMSM_ERR_ARG, "gmsm_debug_reduce_shape: nw >= 1, 1 <= nbuckets <= 2^19");
    Context *ctx;
    int rc = get_context(&ctx);
    if (rc) return rc;
    vt->reduce_shape(*ctx, nw, nbuckets, out);
    return GMSM_OK;
}

GMSM_EXPORT int gmsm_debug_run_layout(int group, int num_cus, size_t n, unsigned c, unsigned win_first, unsigned win_stride, int glv,
                                      int shared, unsigned flags, uint64_t *out) {
    VT_OR_FAIL(group);
    if (num_cus < 1 || num_cus > 4096 || n == 0 || c < 1 || c > 24 || flags > 31 || (flags >> 3) > 2 || !out)
        return fail(GMSM_ERR_ARG, "gmsm_debug_run_layout: 1 <= num_cus <= 4096, n >= 1, 1 <= c <= 24, flags as documented");
    return vt->run_layout(num_cus, n, c, win_first, win_stride, glv != 0, shared != 0, flags, out);
}

GMSM_EXPORT int gmsm_debug_fold_planes(int group, unsigned c, unsigned nwin, unsigned log2L, unsigned nblocks1, const uint64_t *planes,
                                       uint64_t *out_jac) {
    VT_OR_FAIL(group);
    if (c < 2 || c > 24 || nwin == 0 || nwin > 512 || log2L > 8 || nblocks1 == 0 || nblocks1 > 128 || !planes || !out_jac)
        return fail(GMSM_ERR_ARG, "gmsm_debug_fold_planes: 2 <= c <= 24, 1 <= nwin <= 512, log2L <= 8, 1 <= nblocks1 <= 128");
    unsigned nhigh = 0;
    while ((1u << nhigh) < nblocks1) ++nhigh;
    vt->fold_planes(planes, c, nwin, log2L, nhigh, out_jac);
    return GMSM_OK;
}

GMSM_EXPORT unsigned gmsm_num_windows(int group, unsigned c) {
    const GroupVTable *vt = vtable(group);
    return (vt && c) ? num_windows(vt->fr_bits, c) : 0;
}

GMSM_EXPORT int gmsm_window_sums_device(int group, const void *d_points, const void *d_scalars, size_t n, unsigned c,
                                        unsigned win_first, unsigned win_stride, void *hip_stream, uint64_t *out_xyzz) {
    VT_OR_FAIL(group);
    if (c < 2 || c > 20) return fail(GMSM_ERR_ARG, "c out of range (2..20)");
    Context *ctx;
    int rc = enter_owner(d_scalars, &ctx);
    if (rc) return rc;
    return vt->window_sums(*ctx, d_points, d_scalars, n, c, win_first, win_stride, (hipStream_t)hip_stream, out_xyzz, nullptr);
}

GMSM_EXPORT int gmsm_window_sums_enqueue(int group, const void *d_points, uint64_t bases_handle, const void *d_scalars,
                                         size_t n, unsigned c, unsigned win_first, unsigned win_stride, void *hip_stream,
                                         void *d_out_xyzz) {
    VT_OR_FAIL(group);
    if (c < 2 || c > 20) return fail(GMSM_ERR_ARG, "c out of range (2..20)");
    if (!d_out_xyzz) return fail(GMSM_ERR_ARG, "d_out_xyzz is null");
    BasesRef rb;
    if (bases_handle) {
        rb = g_bases.get(bases_handle);
        if (!rb || rb->group != group) return fail(GMSM_ERR_ARG, "unknown bases handle");
        if (n > rb->n) return fail(GMSM_ERR_LEN, "len(points) != len(scalars)");
    }
    Context *ctx;
    int rc = rb ? enter_on(rb->device, &ctx) : enter_owner(d_out_xyzz, &ctx);
    if (rc) return rc;
    // hip_stream is used as given: NULL is the device's default (null) stream, which is what the consumer of d_out_xyzz
    // is ordered against when it runs there too - not the engine's private stream.
    return vt->window_sums_enqueue(*ctx, d_points, d_scalars, n, c, win_first, win_stride, (hipStream_t)hip_stream,
                                   d_out_xyzz, rb);  // the workspace keeps the reference while the work is in flight
}

GMSM_EXPORT int gmsm_fold_window_sets(int group, unsigned c, const uint64_t *xyzz_sets, unsigned nsets, uint64_t *out_jac) {
    VT_OR_FAIL(group);
    if (c < 2 || c > 24) return fail(GMSM_ERR_ARG, "c out of range");
    if (nsets == 0) return fail(GMSM_ERR_ARG, "nsets must be >= 1");
    vt->fold_sets(xyzz_sets, nsets, c, out_jac);
    return GMSM_OK;
}

GMSM_EXPORT int gmsm_fold_windows(int group, unsigned c, const uint64_t *xyzz_windows, uint64_t *out_jac) {
    VT_OR_FAIL(group);
    if (c < 2 || c > 24) return fail(GMSM_ERR_ARG, "c out of range");
    vt->fold(xyzz_windows, c, out_jac);
    return GMSM_OK;
}

GMSM_EXPORT int gmsm_jac_to_affine(int group, const uint64_t *jac, uint64_t *out_affine) {
    VT_OR_FAIL(group);
    vt->jac_to_affine(jac, out_affine);
    return GMSM_OK;
}

GMSM_EXPORT size_t gmsm_affine_limbs(int group) {
    const GroupVTable *vt = vtable(group);
    return vt ? vt->aff_bytes / 8 : 0;
}

GMSM_EXPORT size_t gmsm_scalar_limbs(int group) {
    const GroupVTable *vt = vtable(group);
    return vt ? vt->scalar_bytes / 8 : 0;
}

GMSM_EXPORT int gmsm_debug_decompose(int group, const uint64_t *scalars, size_t n, unsigned c, uint32_t *out_digits) {
    VT_OR_FAIL(group);
    return vt->debug_decompose(scalars, n, c, out_digits);
}

GMSM_EXPORT int gmsm_debug_glv_split(int group, const uint64_t *scalars, size_t n, uint32_t *out) {
    VT_OR_FAIL(group);
    return vt->debug_glv_split(scalars, n, out);
}

GMSM_EXPORT int gmsm_debug_field_op(int group, int field, int op, const uint64_t *a, const uint64_t *b, size_t count,
                                    uint64_t *out) {
    VT_OR_FAIL(group);
    if (count == 0) return GMSM_OK;
    return vt->debug_field_op(field, op, a, b, count, out);
}

GMSM_EXPORT int gmsm_debug_group_op(int group, int op, const uint64_t *acc, const uint64_t *other, size_t count,
                                    uint64_t *out) {
    VT_OR_FAIL(group);
    if (count == 0) return GMSM_OK;
    return vt->debug_group_op(op, acc, other, count, out);
}

GMSM_EXPORT int gmsm_generate_points(int group, const uint64_t *base_affine, const uint64_t *k0, const uint64_t *k1,
                                     int klimbs, size_t n, int nthreads, uint64_t *out_points) {
    VT_OR_FAIL(group);
    if (klimbs < 1 || klimbs > 16) return fail(GMSM_ERR_ARG, "klimbs out of range");
    if (n) vt->generate_points(base_affine, k0, k1, klimbs, n, nthreads, out_points);
    return GMSM_OK;
}

GMSM_EXPORT void gmsm_set_profiling(int on) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_profiling.store(on == 2 ? 2 : on != 0 ? 1 : 0);
    for (int i = 0; i < STAGE_COUNT; ++i) {
        g_stage_ms[i] = 0;
        g_stage_launches[i] = 0;
    }
    g_stage_calls = 0;
}

GMSM_EXPORT int gmsm_get_stage_times(double *out_ms, int max_stages, unsigned long *out_calls) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    int n = max_stages < (int)STAGE_COUNT ? max_stages : (int)STAGE_COUNT;
    for (int i = 0; i < n; ++i) out_ms[i] = g_stage_ms[i];
    if (out_calls) *out_calls = g_stage_calls;
    return n;
}

GMSM_EXPORT int gmsm_get_stage_launches(unsigned long *out_launches, int max_stages) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    int n = max_stages < (int)STAGE_COUNT ? max_stages : (int)STAGE_COUNT;
    for (int i = 0; i < n; ++i) out_launches[i] = g_stage_launches[i];
    return n;
}

GMSM_EXPORT int gmsm_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

GMSM_EXPORT int gmsm_set_device(int device) {
    int n = gmsm_device_count();
    if (device < 0 || device >= n) return fail(GMSM_ERR_DEVICE, "gmsm_set_device: no such device");
    g_device = device;
    g_default_device.store(device);
    g_pinned.store(true);
    return GMSM_OK;
}

GMSM_EXPORT int gmsm_set_devices(const int *devices, int count) {
    std::vector<int> list;
    if (count > 0) {
        if (!devices) return fail(GMSM_ERR_ARG, "gmsm_set_devices: devices is null");
        if (int rc = devices_exist("gmsm_set_devices", devices, (size_t)count, gmsm_device_count())) return rc;
        list.assign(devices, devices + count);
    }
    std::lock_guard<std::mutex> lk(g_devices_mu);
    g_devices = list;
    g_devices_explicit = count > 0;
    if (count > 0) g_default_device.store(list[0]);  // the single-device entries follow the first of them
    else g_pinned.store(false);                      // count = 0: back to the default (GMSM_DEVICES, else no spreading)
    return GMSM_OK;
}

GMSM_EXPORT int gmsm_get_devices(int *out_devices, int max_devices) {
    std::vector<int> list;
    if (shard_devices(list) != GMSM_OK) return -1;  // malformed GMSM_DEVICES: gmsm_last_error() has the text
    if (list.empty()) {  // nothing configured (or pinned): the calling thread's device
        if (out_devices && max_devices > 0) out_devices[0] = g_device >= 0 ? g_device : g_default_device.load();
        return 1;
    }
    if (out_devices)
        for (int i = 0; i < (int)list.size() && i < max_devices; ++i) out_devices[i] = list[i];
    return (int)list.size();
}

// ------------------------------------------------------------------ switches and lifecycle
// One row per key, read by both entries: a key cannot be settable and unreadable. `accepts` null: every value.
struct OptionRow {
    int key;
    std::atomic<unsigned> Options::*member;
    bool (*accepts)(unsigned value);
    const char *refusal;
    bool as_flag = false;  // stored as value != 0
};
static const OptionRow OPTION_ROWS[] = {
    {GMSM_OPT_WINDOW_BITS, &Options::window_bits, [](unsigned v) { return v == 0 || (v >= 2 && v <= 20); },
     "GMSM_OPT_WINDOW_BITS: 0 (the measured table) or 2..20"},
    {GMSM_OPT_TABLES, &Options::tables, [](unsigned v) { return v <= 2; }, "GMSM_OPT_TABLES: 0 never, 1 the measured call sizes, 2 every call size"},
    {GMSM_OPT_MAX_RUN, &Options::max_run, nullptr, nullptr},
    {GMSM_OPT_HOST_RANGES, &Options::host_ranges, nullptr, nullptr},
    {GMSM_OPT_FIXED_BASE_BITS, &Options::fixed_base_bits, [](unsigned v) { return v == 0 || (v >= 2 && v <= 14); },
     "GMSM_OPT_FIXED_BASE_BITS: 0 (by batch size) or 2..14"},
    {GMSM_OPT_SMALL_BITS, &Options::small_bits, [](unsigned v) { return v <= 7; },
     "GMSM_OPT_SMALL_BITS: 0 (on, width by size), 1 (off) or 2..7 (on, forced width)"},
    {GMSM_OPT_SMALL_MAX, &Options::small_max, nullptr, nullptr},
    {GMSM_OPT_SPLIT, &Options::retired_split, nullptr, nullptr, true},  // retired: accepted, no effect
    {GMSM_OPT_GLV, &Options::glv, [](unsigned v) { return v <= 2; }, "GMSM_OPT_GLV: 0 never, 1 where measured ahead, 2 every unregistered call"},
    {GMSM_OPT_SMALL_QUAD, &Options::small_quad, [](unsigned v) { return v <= 2; }, "GMSM_OPT_SMALL_QUAD: 0 by call size, 1 never, 2 always"},
    {GMSM_OPT_POLY_LANE_BITS, &Options::poly_lane_bits, [](unsigned v) { return v <= 6; },
     "GMSM_OPT_POLY_LANE_BITS: 0 (lane width by length) or 1..6 (lanes of 2^(k-1) coefficients)"},
    {GMSM_OPT_REDUCE_SHAPE, &Options::reduce_shape,
     [](unsigned v) { return !(v > 255 || (v & 15u) > 8 || ((v >> 4) & 3u) == 1 || ((v >> 6) & 3u) == 3); },
     "GMSM_OPT_REDUCE_SHAPE: 0 (the cost model) or log2L (0, 1..8) | levels (0, 2, 3) << 4 | combine kernel (0, 1, 2) << 6"},
    {GMSM_OPT_REDUCE_TAIL, &Options::reduce_tail, [](unsigned v) { return v <= 2; },
     "GMSM_OPT_REDUCE_TAIL: 0 by group and call, 1 the device ladder, 2 the host planes"},
    {GMSM_OPT_SPIN_WAIT_US, &Options::spin_wait_us, [](unsigned v) { return v <= 1000000; }, "GMSM_OPT_SPIN_WAIT_US: at most 1000000"},
};
static const OptionRow *option_row(int key) {
    for (const OptionRow &r : OPTION_ROWS)
        if (r.key == key) return &r;
    return nullptr;
}

GMSM_EXPORT int gmsm_set_option(int key, unsigned value) {
    Options &o = options();
    const OptionRow *r = option_row(key);
    if (!r) return fail(GMSM_ERR_ARG, "gmsm_set_option: unknown key");
    if (r->accepts && !r->accepts(value)) return fail(GMSM_ERR_ARG, r->refusal);
    (o.*r->member).store(r->as_flag ? (value ? 1 : 0) : value);
    return GMSM_OK;
}

GMSM_EXPORT unsigned gmsm_get_option(int key) {
    Options &o = options();
    const OptionRow *r = option_row(key);
    return r ? (o.*r->member).load() : 0;
}

// Scratch of the idle workspaces back to the device (the reference's buffers are per call and garbage-collected,
// ecc/bn254/multiexp.go:148-176; ours are grow-only so that a steady stream of calls never allocates - one 2^26 call
// would otherwise pin tens of GB for the life of the process). Workspaces that are leased right now are left alone.
GMSM_EXPORT int gmsm_trim(size_t keep_bytes, size_t *out_freed) {
    if (out_freed) *out_freed = 0;
    std::vector<Context *> ctxs;
    {
        std::lock_guard<std::mutex> lk(g_ctx_mu);
        ctxs = g_ctx;
    }
    int prev = 0;
    (void)hipGetDevice(&prev);
    size_t freed = 0;
    for (Context *c : ctxs) {
        if (!c || !c->live) continue;
        (void)hipSetDevice(c->device);
        // one workspace at a time - lease, drain, trim, release - so that a submit or a blocking entry arriving meanwhile
        // always finds the other workspaces (holding all of them at once turned "trim under load" into spurious
        // "already in flight" errors for unrelated callers)
        for (int i = 0; i < Context::NUM_WS; ++i) {
            Workspace *w = c->acquire_this(i);
            if (!w) continue;  // leased by a running call or a ticket: its scratch is in use
            // an enqueue-only call (gmsm_window_sums_enqueue) may have left work on the caller's stream
            if (w->last_use) (void)hipEventSynchronize(w->last_use);
            if (w->stream) (void)hipStreamSynchronize(w->stream);
            if (w->mstream) (void)hipStreamSynchronize(w->mstream);
            if (w->cstream) (void)hipStreamSynchronize(w->cstream);
            w->conv_pending = false;
            std::shared_ptr<ResidentBases> parked;
            parked.swap(w->bases_ref);
            freed += w->trim(keep_bytes);
            c->release(w);
        }
    }
    (void)hipSetDevice(prev);
    if (out_freed) *out_freed = freed;
    return GMSM_OK;
}

// Everything back: registered bases, FFT domains, workspaces, streams, events, contexts. The library is usable again
// afterwards (contexts reappear on first use). No other call may be running or start while this one runs; outstanding
// tickets are refused (collect them first).
GMSM_EXPORT int gmsm_shutdown(void) {
    std::vector<Context *> ctxs;
    {
        std::lock_guard<std::mutex> lk(g_ctx_mu);
        ctxs = g_ctx;
    }
    // Every workspace of every context is leased FIRST - blocking callers still inside finish, new ones wait behind the
    // lease - and the check for uncollected tickets happens under the same lock as each lease, so no submit can slip in
    // between the check and the teardown (it used to: shutdown then waited for ever on a ticket nobody would collect).
    std::vector<std::pair<Context *, Workspace *>> held;
    for (Context *c : ctxs) {
        if (!c || !c->live) continue;
        for (int i = 0; i < Context::NUM_WS; ++i) {
            Workspace *w = c->acquire_unless_ticket(i);
            if (!w) {
                for (auto &h : held) h.first->release(h.second);
                return fail(GMSM_ERR_ARG, "gmsm_shutdown: a submitted MultiExp has not been collected");
            }
            held.emplace_back(c, w);
        }
    }
    {
        // the memory goes with the last reference, at the end of this block (outside the tables' locks)
        const auto bases = g_bases.drain();
        const auto sharded = g_sharded.drain();
        const auto ffts = g_fft.drain();
        const auto claims = g_gkr.drain();
        const auto trees = g_merkle.drain();
        const auto oracles = g_fri.drain();
    }
    int prev = 0;
    (void)hipGetDevice(&prev);
    for (Context *c : ctxs) {
        if (!c || !c->live) continue;
        (void)hipSetDevice(c->device);
        (void)hipDeviceSynchronize();
        for (auto &w : c->ws) w.destroy();  // all of them are in `held`
        // the leases end here: a caller that was parked on this context's condition variable (a submit or a blocking entry
        // that arrived while everything was leased) wakes into another epoch and returns GMSM_ERR_DEVICE; the Context
        // object itself stays (advisor, round 5: deleting it left such a waiter on a destroyed mutex) and init() runs
        // again on the next use
        c->retire();
    }
    (void)hipSetDevice(prev);
    return GMSM_OK;
}

GMSM_EXPORT const char *gmsm_last_error(void) {
    if (g_last_error.empty()) {  // this thread never failed: hand out the process-wide text (copied, so it stays valid)
        std::lock_guard<std::mutex> lk(g_any_error_mu);
        g_last_error = g_any_error;
    }
    return g_last_error.c_str();
}
GMSM_EXPORT const char *gmsm_version(void) { return "gmsm 0.6 (gfx950)"; }

}  // extern "C"
