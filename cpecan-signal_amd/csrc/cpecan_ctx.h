/*
 * cpecan_ctx.h -- what the files of the C-ABI layer share: the context, its model tables and the small helpers
 * around device memory (cpecan_hip.hip: contexts, the kernel choice and batch creation; cpecan_run.hip: how a run is queued;
 * cpecan_readback.hip: what a finished run gives back; cpecan_models.hip: the model tables).  The batch itself: cpecan_batch.h.  Private to the library: the functions
 * declared here are defined in cpecan_hip.hip and hidden from its exports.
 */
#ifndef CPECAN_CTX_H
#define CPECAN_CTX_H

#include "cpecan_hip.h"
#include "cpecan_device.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

/* (none of this is part of the library's interface: the export list stays what include/cpecan_hip.h declares) */
#pragma GCC visibility push(hidden)

/* The machines a batch can run (the CPECAN_MACHINE_* numbers of cpecan_hip.h): what the context's model tables and the
 * rows of MACHINES[] (cpecan_hip.hip) are indexed by. */
enum Machine {
    STRAWMAN = CPECAN_MACHINE_STRAWMAN, DNA5 = CPECAN_MACHINE_DNA5, VANILLA = CPECAN_MACHINE_VANILLA,
    HDP = CPECAN_MACHINE_HDP, SM4 = CPECAN_MACHINE_SM4, ECHELON = CPECAN_MACHINE_ECHELON, N_MACHINES
};

/* CPECAN_TIMING=1: wall-clock laps of the host-side set-up calls on stderr (where the time before the first kernel goes) */
struct Lap {
    const char *who;
    bool on;
    std::chrono::steady_clock::time_point t, t0;
    explicit Lap(const char *w) : who(w), on(getenv("CPECAN_TIMING") != nullptr), t(std::chrono::steady_clock::now()), t0(t) {}
    ~Lap() {
        if (on)
            fprintf(stderr, "[cpecan timing] %s: TOTAL %.1f ms\n", who,
                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    void operator()(const char *what) {
        if (!on) return;
        const auto n = std::chrono::steady_clock::now();
        fprintf(stderr, "[cpecan timing] %s: %s %.1f ms\n", who, what, std::chrono::duration<double, std::milli>(n - t).count());
        t = n;
    }
};

int host_threads(); /* worker threads for host-side table derivation (cpecan_hip.hip) */
int fail(int code, const char *fmt, ...); /* sets cpecan_hip_last_error(), returns code */

#define HIP_TRY(expr)                                                                        \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess)                                                                \
            return fail(CPECAN_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),  \
                        __FILE__, __LINE__);                                                 \
    } while (0)

/* Device memory of batches and model tables goes through a small caching allocator: hipMalloc and hipFree wait for
 * the device, so a host thread that prepares the next batch while the GPU works on the current one (one-shot
 * alignment of a stream of batches) would otherwise stall on every buffer.  A released block is kept (up to
 * CPECAN_ALLOC_CACHE_GB; by default half of the device's memory -- one process per GPU is the deployment, and RCCL's
 * buffers, torch in the same process or other processes on the card keep the other half; cpecan_hip_trim_cache()
 * gives everything back)
 * and handed to the next request it fits within 25 %.  A block keeps its real size through every reuse. */
struct DevCache {
    struct Block { void *p; size_t bytes; int device; };
    std::mutex lock;
    std::vector<Block> blocks;
    size_t held = 0;
    const bool pinnedHost; /* the same for pinned host memory (the packed pairs of a batch): pinning and unpinning
                              150 MB per batch costs tens of milliseconds; up to CPECAN_PINNED_CACHE_GB, default 8 */
    size_t capBytes = 0; /* 0: not worked out yet */
    explicit DevCache(bool host) : pinnedHost(host) {}
    size_t cap() { /* (under `lock`) */
        if (capBytes == 0) {
            const char *e = getenv(pinnedHost ? "CPECAN_PINNED_CACHE_GB" : "CPECAN_ALLOC_CACHE_GB");
            double gb = e ? atof(e) : 8.0;
            if (!e && !pinnedHost) {
                size_t freeB = 0, totalB = 0;
                /* half the card: three C3 batches on the assembly sweeps (ring of three windows: 45 GB each) alive at once,
                 * as a one-shot service keeps them, still turn over inside the cache */
                gb = hipMemGetInfo(&freeB, &totalB) == hipSuccess ? (double) totalB / 2.0 / (double) (1ull << 30) : 32.0;
            }
            capBytes = (size_t) (gb * (double) (1ull << 30)) + 1;
        }
        return capBytes;
    }
    hipError_t raw_alloc(void **out, size_t bytes) { return pinnedHost ? hipHostMalloc(out, bytes, hipHostMallocDefault) : hipMalloc(out, bytes); }
    void raw_free(void *p) { (void) (pinnedHost ? hipHostFree(p) : hipFree(p)); }
    /* most: no cached block larger than this (the room an account with a limit has left) */
    hipError_t get(void **out, size_t bytes, size_t *got, size_t most = SIZE_MAX) {
        *got = bytes;
        int device = 0;
        (void) hipGetDevice(&device);
        {
            std::lock_guard<std::mutex> g(lock);
            size_t best = blocks.size();
            for (size_t i = 0; i < blocks.size(); i++)
                if (blocks[i].device == device && blocks[i].bytes >= bytes && blocks[i].bytes <= bytes + bytes / 4 + 4096 && blocks[i].bytes <= most &&
                    (best == blocks.size() || blocks[i].bytes < blocks[best].bytes))
                    best = i;
            if (best != blocks.size()) {
                *out = blocks[best].p;
                *got = blocks[best].bytes;
                held -= blocks[best].bytes;
                blocks.erase(blocks.begin() + (long) best);
                return hipSuccess;
            }
        }
        hipError_t e = raw_alloc(out, bytes);
        if (e != hipSuccess) { /* out of memory with blocks in the cache: give them back and try once more */
            trim(0);
            (void) hipGetLastError();
            e = raw_alloc(out, bytes);
        }
        return e;
    }
    void put(void *p, size_t bytes) {
        int device = 0;
        (void) hipGetDevice(&device);
        std::lock_guard<std::mutex> g(lock);
        if (held + bytes > cap()) { /* the cache is bounded (small blocks are kept too: hipFree waits for the device
                                       whatever the size, and the device is busy with the previous batch) */
            raw_free(p);
            return;
        }
        blocks.push_back({ p, bytes, device });
        held += bytes;
    }
    void trim(size_t keep) {
        std::lock_guard<std::mutex> g(lock);
        while (!blocks.empty() && held > keep) {
            raw_free(blocks.back().p);
            held -= blocks.back().bytes;
            blocks.pop_back();
        }
    }
};
DevCache &dev_cache();
DevCache &pinned_cache();

/* a block of pinned host memory from the cache (host-built tables on their way to the device) */
template <typename T> struct PinnedBuf {
    T *p = nullptr;
    size_t n = 0, blockBytes = 0;
    hipError_t alloc(size_t count) {
        release();
        n = count;
        if (count == 0) return hipSuccess;
        return pinned_cache().get((void **) &p, count * sizeof(T), &blockBytes);
    }
    void release() {
        if (p) pinned_cache().put(p, blockBytes);
        p = nullptr;
        n = blockBytes = 0;
    }
    ~PinnedBuf() { release(); }
};

/* Whose device memory it is: one account per context, shared with its batches (a batch may outlive its context).  live:
 * the blocks, at the size the cache handed them out, that the context's model tables and its batches hold now; peak: the
 * most that was since the last reset; limit: 0, none -- otherwise an allocation that would take live past it is refused
 * (cpecan_hip_ctx_set_memory_limit).  A context and its batches are used by one thread at a time, so the counters are
 * plain; what the cache itself keeps of released blocks is nobody's (CPECAN_ALLOC_CACHE_GB bounds that, separately). */
struct MemAccount {
    long long live = 0, peak = 0, limit = 0;
    std::shared_ptr<MemAccount> of; /* a batch's account: its context's, which counts the batch's blocks too */
    /* the account, this one or one it is part of, whose limit `bytes` more would pass (null: none) */
    const MemAccount *refuses(size_t bytes) const {
        for (const MemAccount *a = this; a; a = a->of.get())
            if (a->limit > 0 && a->live + (long long) bytes > a->limit) return a;
        return nullptr;
    }
    size_t room() const { /* the largest block none of them refuses */
        size_t r = SIZE_MAX;
        for (const MemAccount *a = this; a; a = a->of.get())
            if (a->limit > 0) r = std::min(r, (size_t) std::max(a->limit - a->live, 0ll));
        return r;
    }
    void take(size_t bytes) {
        for (MemAccount *a = this; a; a = a->of.get()) {
            a->live += (long long) bytes;
            if (a->live > a->peak) a->peak = a->live;
        }
    }
    void give(size_t bytes) {
        for (MemAccount *a = this; a; a = a->of.get()) a->live -= (long long) bytes;
    }
};
/* The account that the calling thread's DevBuf allocations go on, for the length of a C-ABI call made on behalf of a
 * context or one of its batches (none: the allocation is nobody's, as the self-test's). */
std::shared_ptr<MemAccount> &mem_current();
struct MemScope {
    std::shared_ptr<MemAccount> outer;
    explicit MemScope(const std::shared_ptr<MemAccount> &a);
    ~MemScope();
};
/* a DevBuf allocation was refused by its account's limit: fail() turns the CPECAN_EHIP of the hipErrorOutOfMemory that
 * alloc() returned into CPECAN_ELIMIT and says what was asked for */
void mem_refused(size_t asked, const MemAccount &a);

template <typename T> struct DevBuf {
    T *p = nullptr;
    size_t n = 0, blockBytes = 0;
    std::shared_ptr<MemAccount> account; /* whose the block is (null: nobody's) */
    hipError_t alloc(size_t count) {
        release();
        if (count == 0) return hipSuccess;
        const std::shared_ptr<MemAccount> &a = mem_current();
        if (a && a->refuses(count * sizeof(T))) {
            mem_refused(count * sizeof(T), *a->refuses(count * sizeof(T)));
            return hipErrorOutOfMemory;
        }
        /* (a cached block is up to a quarter larger than what was asked for: none that the account has no room for) */
        const hipError_t e = dev_cache().get((void **) &p, count * sizeof(T), &blockBytes, a ? a->room() : SIZE_MAX);
        if (e != hipSuccess) { /* a buffer that could not be had is an empty one: `n` never speaks of a block that is not there */
            p = nullptr;
            blockBytes = 0;
            return e;
        }
        n = count;
        if (a) {
            a->take(blockBytes);
            account = a;
        }
        return e;
    }
    void release() {
        if (p) dev_cache().put(p, blockBytes);
        if (p && account) account->give(blockBytes);
        account.reset();
        p = nullptr;
        n = blockBytes = 0;
    }
    void swap(DevBuf &o) {
        std::swap(p, o.p);
        std::swap(n, o.n);
        std::swap(blockBytes, o.blockBytes);
        std::swap(account, o.account);
    }
    ~DevBuf() { release(); }
};

/* Declared after a function's own DevBuf / PinnedBuf objects and before its first asynchronous use of them: whichever
 * way the function returns, the streams it fed are idle before those buffers go back to the cache (a released block
 * can be handed to another thread at once; hipFree used to wait for the device here). */
struct StreamFence {
    hipStream_t a = nullptr, b = nullptr;
    ~StreamFence() {
        if (a) (void) hipStreamSynchronize(a);
        if (b) (void) hipStreamSynchronize(b);
    }
};

struct LaneSet; /* the three streams a chain of batches runs on (cpecan_batch.h, cpecan_run.hip) */
struct cpecan_ctx;

/* The models of one machine in a context: blocks of `stride` doubles next to each other on the device (no host mirror
 * of them is kept), a model's id its place in the table, and one double per model that the host still needs (`side`).
 * Batches hold ids, never the block's address, which every run reads afresh: a table may grow under a live batch.
 *
 * What a create call leaves behind when it fails (cpecan_models.hip), the same for all six machines:
 *   - a call that fails before its rows are on the device, grow() included, leaves the table as it found it: block,
 *     count, side values and every id handed out earlier stay valid;
 *   - a call whose upload goes wrong after grow() has swapped the blocks cannot tell what the new block holds: it
 *     drops the table and bumps the context's modelEpoch, as cpecan_hip_models_clear does, so that batches created
 *     earlier are refused instead of reading ids into a table that is gone.
 * Count and side values change in commit() and drop() alone (cpecan_hip_models_set_transitions rewrites the strawMan
 * side values in place, with the tables). */
struct ModelTable {
    const size_t stride; /* doubles per model */
    DevBuf<double> block; /* n * stride */
    int n = 0;
    std::vector<double> side; /* strawMan and HDP: the model's GAP_SWITCH_TO_X (which sweep build a batch runs);
                                 vanilla: its m_to_y_not_x, which the skip bins' logs depend on; the others: unused */
    /* room for `more` models at the end: a new block, the old rows copied across on the device; *fresh receives the
     * device address of the first new model.  The count stays: the new rows are not models before commit(). */
    int grow(cpecan_ctx *c, int32_t more, double **fresh);
    /* the rows grow() made room for are on the device: they are models now, ids[i] theirs */
    void commit(int32_t more, const double *sideValues, int32_t *ids) {
        for (int i = 0; i < more; i++) ids[i] = n + i;
        side.insert(side.end(), sideValues, sideValues + more);
        n += more;
    }
    /* the table is empty again (the caller has waited for its readers: ctx_fence) */
    void drop() {
        block.release();
        side.clear();
        n = 0;
    }
};

#define CP_HDP_MODEL_DOUBLES 14 /* one DevHdpModel record, the stride of the HDP table */
static_assert(sizeof(DevHdpModel) == CP_HDP_MODEL_DOUBLES * sizeof(double), "the HDP table is kept as doubles");

struct cpecan_ctx {
    int device = 0;
    std::shared_ptr<MemAccount> mem = std::make_shared<MemAccount>(); /* its model tables and its batches (MemScope) */
    long long modelEpoch = 0; /* counts cpecan_hip_models_clear calls (and tables dropped by a failed upload) */
    LaneSet *lanes = nullptr;
    hipStream_t stream = nullptr; /* lanes->fwd */
    std::vector<cpecan_batch *> batches; /* its live batches (under g_batchesMu): ctx_fence waits for their runs */
    /* input preparation (uploads, table assembly, k-mer indices) goes through a stream of the highest priority: it
     * gets a hardware queue of its own and its copies and small kernels are not held up behind the sweeps of the
     * batches that are running while the next one is prepared; every call that uses it waits for it before it returns */
    hipStream_t prep = nullptr;
    void *pinned = nullptr; /* staging slots of the threaded model creates (pinned_slots) */
    size_t pinnedBytes = 0;
    /* per machine: strawMan tables; 5-state symbol models; vanilla blocks; HDP descriptors (DevHdpModel); 4-state
     * models (strawMan tables whose header holds eleven transitions); echelon blocks */
    ModelTable tables[N_MACHINES] = { { CP_MODEL_STRIDE }, { CP_MODEL5_STRIDE }, { CP_VMODEL_STRIDE },
                                      { CP_HDP_MODEL_DOUBLES }, { CP_MODEL_STRIDE }, { CP_EMODEL_STRIDE } };
    /* what the HDP descriptors point to: every model's tables in buffers of their own */
    struct HdpTables {
        DevBuf<int> kmerRow;
        DevBuf<double> grid, y, slope;
    };
    std::vector<HdpTables *> hdpTables;
    std::string hdpAlphabet;
};

/* every run of the context's batches is over: what guards the model tables those runs read (cpecan_hip.hip) */
hipError_t ctx_fence(cpecan_ctx *c);
/* the context's pinned staging slots, at least `want` bytes */
int pinned_slots(cpecan_ctx *c, size_t want);

#pragma GCC visibility pop

#endif
