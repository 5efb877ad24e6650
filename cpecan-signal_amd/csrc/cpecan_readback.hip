/*
 * cpecan_readback.hip -- from a finished run to the caller's counts and pairs: the two kernels that pack a run's
 * candidates for the host, the pack at the end of a run, and the readback calls of include/cpecan_hip.h.
 *
 * The device selects pairs by the exponent (F+B)-total with a margin below log(threshold); exp(), the exact threshold
 * test and floor(p * 1e7) are finished here with the host libm, the one the reference calls
 * (diagonalCalculationPosteriorMatchProbs, impl/pairwiseAligner.c:776-786).  What of that needs no device is in
 * cpecan_readback_host.h.
 */
#include "cpecan_batch.h"

#include "cpecan_readback_host.h"

#include <atomic>
#include <cstring>
#include <thread>

/* Item i's first packBase[i + 1] - packBase[i] candidates, from its own region of the pair buffers to the packed one.
 * With every candidate goes a verdict on its integer posterior: the device's exp() and the host libm's differ by at
 * most a few units in the last place, so wherever exp(logp) is not within a (far wider) margin of the threshold, of 1
 * or of a multiple of 1e-7, floor(p * 1e7) is the same number on both and is taken here (post >= 0), or the pair is
 * surely below the threshold (post -2); the few that are close (post -1) are finished by the host with its libm. */
extern "C" __global__ void cpecan_k_pack_pairs(const DevItem *items, const long long *packBase, const long long *pairs,
                                               const double *logp, double threshold, long long capacity,
                                               PackedPair *out, int *post, long long *undecided /* [0] count, then
                                               CP_UNDECIDED_CAP x (packed index, exponent bits) */,
                                               int compact /* both coordinates below 65536: four bytes a pair */) {
    const DevItem &d = items[blockIdx.x];
    if (packBase[gridDim.x] > capacity) return; /* (packed at the end of a run into a buffer sized by a guess: the host
                                                   sees the same total and packs again into one that fits) */
    const long long o = packBase[blockIdx.x], n = packBase[blockIdx.x + 1] - o;
    for (long long k = threadIdx.x; k < n; k += blockDim.x) {
        PackedPair r;
        r.x = (int) pairs[(d.pairBase + k) * 3 + 1];
        r.y = (int) pairs[(d.pairBase + k) * 3 + 2];
        if (compact) ((unsigned *) out)[o + k] = (unsigned) r.x | ((unsigned) r.y << 16);
        else out[o + k] = r;
        const double e = logp[d.pairBase + k];
        const double p = exp(e);
        int v = -1;
        if (p == p) {
            if (p < threshold - (1e-9 * threshold + 1e-300)) v = -2;
            else if (p > threshold + (1e-9 * threshold + 1e-300) || threshold == 0.0) {
                if (p > 1.0 + 1e-9) v = 10000000;
                else if (p < 1.0 - 1e-9) {
                    const double q = p * 10000000.0, fl = floor(q);
                    if (q - fl > 1e-5 && fl + 1.0 - q > 1e-5) v = (int) fl;
                } else if (e >= 0.0) v = 10000000; /* exp(e) >= 1 on any libm: clamped to 1 */
                else if (e <= -1e-15) v = 9999999; /* exp(e) <= 1 - 9e-16 < 1, and p * 1e7 rounds below 1e7 (its
                                                      ulp there is 1.9e-9, the deficit at least 1e-8): a quarter of a
                                                      C3 batch's candidates are this sure a match */
            }
        }
        post[o + k] = v;
        if (v == -1) { /* the host settles it: its exponent goes along (a short list; a batch that overflows it has
                          the host fetch the exponents item by item) */
            const unsigned long long j = atomicAdd((unsigned long long *) undecided, 1ull);
            if (j < CP_UNDECIDED_CAP) {
                undecided[1 + 2 * j] = o + k;
                undecided[2 + 2 * j] = __double_as_longlong(e);
            }
        }
    }
}

/* packBase[i] = candidates of the items before i (each item's count capped at its capacity), packBase[n] = all of
 * them: the offsets cpecan_k_pack_pairs writes to, formed on the device so that a run can end with its candidates
 * packed (the host forms the same sums from the counts it fetches) */
extern "C" __global__ __launch_bounds__(256) void cpecan_k_pack_base(const DevItem *items, const long long *nPairs,
                                                                     long long nItems, long long *packBase) {
    __shared__ long long part[256];
    const long long per = (nItems + 255) / 256, i0 = threadIdx.x * per, i1 = i0 + per < nItems ? i0 + per : nItems;
    long long sum = 0;
    for (long long i = i0; i < i1; i++) sum += nPairs[i] < items[i].pairCap ? nPairs[i] : items[i].pairCap;
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long run = 0;
        for (int t = 0; t < 256; t++) {
            const long long v = part[t];
            part[t] = run;
            run += v;
        }
        packBase[nItems] = run;
    }
    __syncthreads();
    long long run = part[threadIdx.x];
    for (long long i = i0; i < i1; i++) {
        packBase[i] = run;
        run += nPairs[i] < items[i].pairCap ? nPairs[i] : items[i].pairCap;
    }
}

/* out[i] = the models' blocks of an E-step's sums added at element i, in ascending model id from block 0's value on:
 * ((e[0][i] + e[1][i]) + e[2][i]) + ..., the sum a host forms that fetches the blocks one by one.  The order is the
 * call's contract (cpecan_hip_batch_sum_expectations), so the adds stay one chain; what runs ahead of it are the loads,
 * eight blocks at a time, each of them coalesced across i.  One thread per element. */
#define CP_SUM_LOADS 8
extern "C" __global__ __launch_bounds__(256) void cpecan_k_sum_expectations(const double *expect, int nModels, int expectLen,
                                                                            double *out) {
    const int i = (int) (blockIdx.x * 256 + threadIdx.x);
    if (i >= expectLen) return; /* (the last block is partly idle: 4106 elements of the strawMan machine) */
    const double *e = expect + i;
    double sum = e[0];
    int k = 1;
    for (; k + CP_SUM_LOADS <= nModels; k += CP_SUM_LOADS) {
        double v[CP_SUM_LOADS];
#pragma unroll
        for (int u = 0; u < CP_SUM_LOADS; u++) v[u] = e[(size_t) (k + u) * (size_t) expectLen];
#pragma unroll
        for (int u = 0; u < CP_SUM_LOADS; u++) sum += v[u];
    }
    for (; k < nModels; k++) sum += e[(size_t) k * (size_t) expectLen];
    out[i] = sum;
}

/* The pack step's device buffers: the offsets, the list of close calls and, for at least `need` candidates, the packed
 * records and verdicts (`capacity` of them where those have to be made or grow). */
static int pack_buffers(cpecan_batch *b, size_t need, size_t capacity) {
    if (b->packBase.n < (size_t) b->nItems + 1) HIP_TRY(b->packBase.alloc((size_t) b->nItems + 1));
    if (b->packed.n < need) { /* (`packed`, which is asked, last: a call that fails half-way is made again in full) */
        b->packed.release();
        HIP_TRY(b->packedPost.alloc(capacity));
        HIP_TRY(b->packed.alloc(capacity));
    }
    if (b->undecided.n == 0) HIP_TRY(b->undecided.alloc(1 + 2 * CP_UNDECIDED_CAP));
    return CPECAN_OK;
}

/* the candidates packed at the offsets b->packBase holds by then on that stream, the list of close calls begun afresh */
static int launch_pack(cpecan_batch *b, hipStream_t st) {
    HIP_TRY(hipMemsetAsync(b->undecided.p, 0, sizeof(long long), st));
    hipLaunchKernelGGL(cpecan_k_pack_pairs, dim3((unsigned) b->nItems), dim3(256), 0, st, (const DevItem *) b->items.p,
                       (const long long *) b->packBase.p, (const long long *) b->pairs.p, (const double *) b->pairLogp.p,
                       b->P.threshold, (long long) b->packed.n, b->packed.p, b->packedPost.p, b->undecided.p,
                       b->compactPairs ? 1 : 0);
    HIP_TRY(hipGetLastError());
    return CPECAN_OK;
}

/* Posterior decode: the run ends with its candidates packed for the host (4- or 8-byte records + the device's verdict),
 * into a buffer sized by a guess the first time (about one candidate per diagonal) and by ensure_counts afterwards,
 * which packs again if the buffer was short.  Done here, inside the pass, because a kernel launched later would wait for
 * wave slots behind the next batch's sweeps. */
int pack_in_run(cpecan_batch *b, hipStream_t sEnd) {
    b->packedInRun = false;
    static const bool packInRun = getenv("CPECAN_PACK_LATER") == nullptr;
    if (!packInRun || b->mode != CPECAN_MODE_POSTERIOR || b->P.debug) return CPECAN_OK;
    long long guess = 0;
    if (b->packed.n == 0)
        for (const DevItem &d : b->hItems) guess += std::min<long long>(d.pairCap, d.lX + d.lY + 64);
    int rc = pack_buffers(b, 1 /* whatever there is will do */, (size_t) guess);
    if (rc != CPECAN_OK) return rc;
    hipLaunchKernelGGL(cpecan_k_pack_base, dim3(1), dim3(256), 0, sEnd, (const DevItem *) b->items.p,
                       (const long long *) b->nPairs.p, (long long) b->nItems, b->packBase.p);
    if ((rc = launch_pack(b, sEnd)) == CPECAN_OK) b->packedInRun = true;
    return rc;
}

void release_readback(cpecan_batch *b) {
    if (b->hPacked) pinned_cache().put(b->hPacked, b->hPackedBlock);
    if (b->hPost) pinned_cache().put(b->hPost, b->hPostBlock);
    if (b->hUndecided) pinned_cache().put(b->hUndecided, b->hUndecidedBlock);
}

/* The steps of ensure_counts, in its order.  Readbacks wait for the run's end event and go through the context's prep
 * stream: the lanes the run went on may carry the next batch's run already. */

/* The run is over and every item's pairs fit its share of the pair buffer.  If an alignment produced more pairs than
 * its share holds (flat posteriors: a tiny threshold, the HDP machine's linear densities), the buffer is re-laid-out to
 * the reported counts and the batch is run once more -- the reference returns the list whatever its length. */
/* The pair buffer as the items' shares (pairCap, pairBase in hItems) now want it, and the items on the device.  A call
 * that a memory limit refuses leaves the batch without the buffer and says so in pairsLaidOut: the next run makes it,
 * and the next readback runs the batch again before it reads anything (ensure_counts). */
int lay_out_pairs(cpecan_batch *b) {
    long long total = 0;
    for (const DevItem &d : b->hItems) total += d.pairCap;
    b->pairsLaidOut = false;
    HIP_TRY(b->pairs.alloc((size_t) total * 3));
    HIP_TRY(b->pairLogp.alloc((size_t) total));
    HIP_TRY(hipMemcpy(b->items.p, b->hItems.data(), (size_t) b->nItems * sizeof(DevItem), hipMemcpyHostToDevice));
    b->pairsLaidOut = true;
    return CPECAN_OK;
}

static int fit_pair_buffer(cpecan_batch *b) {
    b->hNPairs.resize((size_t) b->nItems);
    b->hNTot.resize((size_t) b->nItems);
    for (int attempt = 0;; attempt++) {
        HIP_TRY(hipEventSynchronize(b->ev2));
        HIP_TRY(hipMemcpy(b->hNPairs.data(), b->nPairs.p, (size_t) b->nItems * sizeof(long long), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(b->hNTot.data(), b->nTot.p, (size_t) b->nItems * sizeof(long long), hipMemcpyDeviceToHost));
        bool over = false;
        for (int64_t i = 0; i < b->nItems; i++)
            if (b->hNPairs[(size_t) i] > b->hItems[(size_t) i].pairCap) over = true;
        if (!over) return CPECAN_OK;
        if (attempt == 2) return fail(CPECAN_EOVERFLOW, "aligned-pair counts keep growing between identical runs");
        long long total = 0;
        for (int64_t i = 0; i < b->nItems; i++) {
            DevItem &d = b->hItems[(size_t) i];
            d.pairCap = std::max(d.pairCap, b->hNPairs[(size_t) i] + 64);
            d.pairBase = total;
            total += d.pairCap;
        }
        int rc = lay_out_pairs(b);
        if (rc == CPECAN_OK) rc = cpecan_hip_batch_run(b);
        if (rc != CPECAN_OK) return rc;
    }
}

/* where every item's candidates begin among those of the batch (what cpecan_k_pack_base forms on the device) */
static int form_pair_base(cpecan_batch *b) {
    b->hPairBase.assign((size_t) b->nItems + 1, 0);
    for (int64_t i = 0; i < b->nItems; i++)
        b->hPairBase[(size_t) i + 1] = b->hPairBase[(size_t) i] + std::min(b->hNPairs[(size_t) i], b->hItems[(size_t) i].pairCap);
    return CPECAN_OK;
}

/* E-step: the lists as they are (in expectation mode the HDP machine's pair buffer carries event-to-k-mer assignments,
 * not posteriors: short lists), those assignments put into the reference's order (order_assignments) */
static int fetch_lists(cpecan_batch *b) {
    hipStream_t rs = b->ctx->prep;
    const long long all = b->hPairBase[(size_t) b->nItems];
    b->hPairs.resize((size_t) all * 3);
    b->hLogp.resize((size_t) all);
    for (int64_t i = 0; i < b->nItems; i++) {
        const DevItem &d = b->hItems[(size_t) i];
        const long long n = b->hPairBase[(size_t) i + 1] - b->hPairBase[(size_t) i], o = b->hPairBase[(size_t) i];
        if (n == 0) continue;
        HIP_TRY(hipMemcpyAsync(b->hPairs.data() + o * 3, b->pairs.p + d.pairBase * 3, (size_t) n * 3 * sizeof(long long),
                               hipMemcpyDeviceToHost, rs));
        HIP_TRY(hipMemcpyAsync(b->hLogp.data() + o, b->pairLogp.p + d.pairBase, (size_t) n * sizeof(double),
                               hipMemcpyDeviceToHost, rs));
    }
    HIP_TRY(hipStreamSynchronize(rs));
    /* the HDP machine's event assignments from the wave kernels come in the order their threads got there */
    if (b->machine == HDP && b->kernel == CPECAN_KERNEL_SYSTOLIC)
        for (int64_t i = 0; i < b->nItems; i++) {
            const long long o = b->hPairBase[(size_t) i], n = b->hPairBase[(size_t) i + 1] - o;
            order_assignments(b->hPairs.data() + o * 3, b->hLogp.data() + o, n);
        }
    return CPECAN_OK;
}

/* Posterior decode: the candidates of all items, packed on the device into one buffer (by the run itself, or now from
 * the host's offsets into a buffer with an eighth to spare), come to pinned memory in one piece each: records,
 * verdicts, close calls. */
static int fetch_packed(cpecan_batch *b) {
    hipStream_t rs = b->ctx->prep;
    const long long all = b->hPairBase[(size_t) b->nItems];
    if (all == 0) return CPECAN_OK;
    const bool packedAlready = b->packedInRun && (size_t) all <= b->packed.n; /* the run ended with them packed */
    const size_t roomy = (size_t) all + (size_t) all / 8;
    int rc = pack_buffers(b, (size_t) all, roomy);
    if (rc != CPECAN_OK) return rc;
    if (b->hPackedCap < (size_t) all) {
        if (b->hPacked) pinned_cache().put(b->hPacked, b->hPackedBlock);
        if (b->hPost) pinned_cache().put(b->hPost, b->hPostBlock);
        b->hPacked = nullptr;
        b->hPost = nullptr;
        b->hPackedCap = roomy;
        HIP_TRY(pinned_cache().get((void **) &b->hPacked, b->hPackedCap * sizeof(PackedPair), &b->hPackedBlock));
        HIP_TRY(pinned_cache().get((void **) &b->hPost, b->hPackedCap * sizeof(int), &b->hPostBlock));
    }
    if (!b->hUndecided)
        HIP_TRY(pinned_cache().get((void **) &b->hUndecided, (1 + 2 * CP_UNDECIDED_CAP) * sizeof(long long), &b->hUndecidedBlock));
    if (!packedAlready) {
        HIP_TRY(hipMemcpyAsync(b->packBase.p, b->hPairBase.data(), ((size_t) b->nItems + 1) * sizeof(long long),
                               hipMemcpyHostToDevice, rs));
        if ((rc = launch_pack(b, rs)) != CPECAN_OK) return rc;
    }
    HIP_TRY(hipMemcpyAsync(b->hUndecided, b->undecided.p, (1 + 2 * CP_UNDECIDED_CAP) * sizeof(long long),
                           hipMemcpyDeviceToHost, rs));
    HIP_TRY(hipMemcpyAsync(b->hPacked, b->packed.p, (size_t) all * (b->compactPairs ? sizeof(unsigned) : sizeof(PackedPair)),
                           hipMemcpyDeviceToHost, rs));
    HIP_TRY(hipMemcpyAsync(b->hPost, b->packedPost.p, (size_t) all * sizeof(int), hipMemcpyDeviceToHost, rs));
    HIP_TRY(hipStreamSynchronize(rs));
    return CPECAN_OK;
}

/* The close calls: settled with the host's libm (settle_exponent), written back over the device's "undecided" verdict;
 * and the number of pairs every item keeps.  The records stay packed in pinned memory; cpecan_hip_batch_fetch_pairs
 * expands an item's pairs into the reference's triples when they are asked for.  Items are independent: dealt to the
 * host threads in contiguous runs of about the same number of candidates each. */
static int settle_close_calls(cpecan_batch *b) {
    const long long all = b->hPairBase[(size_t) b->nItems];
    const double threshold = b->P.threshold;
    int *verdict = b->hPost;
    static const bool hostOnly = getenv("CPECAN_HOST_FINALISE") != nullptr; /* (tests: every pair through the host libm) */
    const int nt = (int) std::min<int64_t>(all > 200000 ? host_threads() : 1, b->nItems);
    const std::vector<int64_t> cut = cut_items(b->hPairBase.data(), b->nItems, nt);
    /* what the device settled is counted by the host threads; what it left open (verdict -1) comes with its exponent
     * in the short list the pack kernel made, and is settled here */
    const long long listed = all > 0 ? b->hUndecided[0] : 0;
    const bool byList = !hostOnly && listed <= (long long) CP_UNDECIDED_CAP;
    if (getenv("CPECAN_TIMING")) fprintf(stderr, "[cpecan timing] ensure_counts: %lld candidates, %lld left to the host\n", all, listed);
    if (byList)
        for (long long j = 0; j < listed; j++) {
            double e;
            memcpy(&e, &b->hUndecided[2 + 2 * j], sizeof e);
            verdict[b->hUndecided[1 + 2 * j]] = settle_exponent(e, threshold);
        }
    std::atomic<int> failed{0};
    auto scan = [b, verdict, byList, threshold, &failed](int64_t i0, int64_t i1) {
        std::vector<double> e;
        for (int64_t i = i0; i < i1; i++) {
            const long long o = b->hPairBase[(size_t) i], n = b->hPairBase[(size_t) i + 1] - o;
            if (!byList && n > 0) { /* (tests, or more close calls than the list holds: this item's exponents from HBM) */
                e.resize((size_t) n);
                if (hipSetDevice(b->ctx->device) != hipSuccess ||
                    hipMemcpy(e.data(), b->pairLogp.p + b->hItems[(size_t) i].pairBase, (size_t) n * sizeof(double),
                              hipMemcpyDeviceToHost) != hipSuccess) {
                    failed = 1;
                    return;
                }
            }
            long long kept = 0;
            for (long long k = 0; k < n; k++) {
                if (!byList && (hostOnly || verdict[o + k] == -1)) verdict[o + k] = settle_exponent(e[(size_t) k], threshold);
                kept += verdict[o + k] >= 0;
            }
            b->hNPairs[(size_t) i] = kept;
        }
    };
    {
        std::vector<std::thread> pool;
        for (int t = 1; t < nt; t++)
            if (cut[(size_t) t + 1] > cut[(size_t) t]) pool.emplace_back(scan, cut[(size_t) t], cut[(size_t) t + 1]);
        scan(cut[0], cut[1]);
        for (std::thread &th : pool) th.join();
    }
    if (failed) return fail(CPECAN_EHIP, "fetching the candidates' exponents failed: %s", hipGetErrorString(hipGetLastError()));
    return CPECAN_OK;
}

/* Counts and aligned pairs of a finished run, once per run. */
static int ensure_counts(cpecan_batch *b) {
    if (!b->pairsLaidOut) {
        /* an earlier readback grew the items' shares of the pair buffer and a memory limit refused the buffer: there is
         * none, and what the last run left is laid out by the old shares.  The run that growth was for, now (it makes
         * the buffer first); where the limit still refuses it, this call fails as that one did */
        const int rc = cpecan_hip_batch_run(b);
        if (rc != CPECAN_OK) return rc;
    }
    if (!b->ran) return fail(CPECAN_EINVAL, "batch has not run");
    if (b->countsValid) return CPECAN_OK;
    HIP_TRY(hipSetDevice(b->ctx->device));
    MemScope mem(b->mem);
    Lap lap("ensure_counts");
    const bool estep = b->mode != CPECAN_MODE_POSTERIOR;
    int rc = fit_pair_buffer(b);
    if (rc == CPECAN_OK) rc = form_pair_base(b);
    if (rc == CPECAN_OK) rc = estep ? fetch_lists(b) : fetch_packed(b);
    if (rc == CPECAN_OK && !estep) rc = settle_close_calls(b);
    b->countsValid = rc == CPECAN_OK;
    return rc;
}

extern "C" {

int cpecan_hip_batch_counts(cpecan_batch *b, int64_t *nPairs, int64_t *nTotals, int64_t *nCells) {
    if (!b) return fail(CPECAN_EINVAL, "batch is NULL");
    int rc = ensure_counts(b);
    if (rc) return rc;
    for (int64_t i = 0; i < b->nItems; i++) {
        if (nPairs) nPairs[i] = b->hNPairs[(size_t) i];
        if (nTotals) nTotals[i] = b->hNTot[(size_t) i];
        if (nCells) nCells[i] = b->hNCells[(size_t) i];
    }
    return CPECAN_OK;
}

int cpecan_hip_batch_fetch_pairs(cpecan_batch *b, int64_t item, int64_t *triples, double *logp,
                                 int64_t cap) {
    if (!b || item < 0 || item >= b->nItems || !triples) return fail(CPECAN_EINVAL, "bad argument");
    int rc = ensure_counts(b);
    if (rc) return rc;
    const long long n = b->hNPairs[(size_t) item], o = b->hPairBase[(size_t) item];
    if (n > cap) return fail(CPECAN_EOVERFLOW, "need room for %lld triples", n);
    if (n == 0) return CPECAN_OK;
    if (b->mode != CPECAN_MODE_POSTERIOR) {
        memcpy(triples, b->hPairs.data() + o * 3, (size_t) n * 3 * sizeof(long long));
        if (logp) memcpy(logp, b->hLogp.data() + o, (size_t) n * sizeof(double));
        return CPECAN_OK;
    }
    /* the item's packed candidates with their settled verdicts -> (floor(p * 1e7), x, y), emission order */
    const long long cand = b->hPairBase[(size_t) item + 1] - o;
    std::vector<double> e;
    if (logp) { /* the exponents stayed in HBM: this item's, now */
        e.resize((size_t) cand);
        HIP_TRY(hipSetDevice(b->ctx->device));
        HIP_TRY(hipMemcpy(e.data(), b->pairLogp.p + b->hItems[(size_t) item].pairBase, (size_t) cand * sizeof(double),
                          hipMemcpyDeviceToHost));
    }
    long long kept = 0;
    for (long long k = 0; k < cand; k++) {
        const int v = b->hPost[o + k];
        if (v < 0) continue;
        triples[kept * 3] = v;
        if (b->compactPairs) {
            const unsigned xy = ((const unsigned *) b->hPacked)[o + k];
            triples[kept * 3 + 1] = xy & 0xFFFFu;
            triples[kept * 3 + 2] = xy >> 16;
        } else {
            triples[kept * 3 + 1] = b->hPacked[o + k].x;
            triples[kept * 3 + 2] = b->hPacked[o + k].y;
        }
        if (logp) logp[kept] = e[(size_t) k];
        kept++;
    }
    return CPECAN_OK;
}

int cpecan_hip_batch_fetch_totals(cpecan_batch *b, int64_t item, int64_t *xay, double *total,
                                  int64_t cap) {
    if (!b || item < 0 || item >= b->nItems) return fail(CPECAN_EINVAL, "bad argument");
    int rc = ensure_counts(b);
    if (rc) return rc;
    const DevItem &d = b->hItems[(size_t) item];
    long long n = b->hNTot[(size_t) item];
    if (n > d.totCap) return fail(CPECAN_EOVERFLOW, "totals overflow (%lld > %lld)", n, d.totCap);
    if (n > cap) return fail(CPECAN_EOVERFLOW, "need room for %lld totals", n);
    if (n == 0) return CPECAN_OK;
    if (xay)
        HIP_TRY(hipMemcpy(xay, b->totXay.p + d.totBase, (size_t) n * sizeof(long long), hipMemcpyDeviceToHost));
    if (total)
        HIP_TRY(hipMemcpy(total, b->totVal.p + d.totBase, (size_t) n * sizeof(double), hipMemcpyDeviceToHost));
    return CPECAN_OK;
}

int cpecan_hip_batch_expectations_device_ptr(cpecan_batch *b, void **devPtr, int64_t *nDoubles) {
    if (!b || !devPtr) return fail(CPECAN_EINVAL, "bad argument");
    *devPtr = (void *) b->expect.p;
    if (nDoubles) *nDoubles = (int64_t) b->expect.n;
    return CPECAN_OK;
}

int cpecan_hip_batch_fetch_expectations(cpecan_batch *b, int32_t modelId, double *out) {
    if (!b || !out || modelId < 0 || modelId >= b->nModels) return fail(CPECAN_EINVAL, "bad argument");
    HIP_TRY(hipSetDevice(b->ctx->device));
    if (b->ran) HIP_TRY(hipEventSynchronize(b->ev2));
    HIP_TRY(hipMemcpy(out, b->expect.p + (size_t) modelId * b->expectLen, (size_t) b->expectLen * sizeof(double),
                      hipMemcpyDeviceToHost));
    return CPECAN_OK;
}

int cpecan_hip_batch_sum_expectations(cpecan_batch *b, double *out) {
    if (!b || !out) return fail(CPECAN_EINVAL, "bad argument");
    if (b->mode != CPECAN_MODE_EXPECTATIONS || b->nModels < 1)
        return fail(CPECAN_EINVAL, "the batch has no expectations (it was not created for an E-step)");
    HIP_TRY(hipSetDevice(b->ctx->device));
    MemScope mem(b->mem);
    Lap lap("sum_expectations");
    if (b->expectSum.n < (size_t) b->expectLen) HIP_TRY(b->expectSum.alloc((size_t) b->expectLen));
    /* behind the run's end event, on the context's prep stream like the other readbacks: one kernel, one copy, one wait */
    hipStream_t rs = b->ctx->prep;
    if (b->ran) HIP_TRY(hipStreamWaitEvent(rs, b->ev2, 0));
    hipLaunchKernelGGL(cpecan_k_sum_expectations, dim3((unsigned) ((b->expectLen + 255) / 256)), dim3(256), 0, rs,
                       (const double *) b->expect.p, b->nModels, b->expectLen, b->expectSum.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, b->expectSum.p, (size_t) b->expectLen * sizeof(double), hipMemcpyDeviceToHost, rs));
    HIP_TRY(hipStreamSynchronize(rs));
    return CPECAN_OK;
}

int cpecan_hip_batch_debug_cells(cpecan_batch *b, int64_t item, double *forward, double *backward,
                                 int64_t nCells) {
    if (!b || item < 0 || item >= b->nItems) return fail(CPECAN_EINVAL, "bad argument");
    if (!b->P.debug || b->kernel != CPECAN_KERNEL_GENERAL)
        return fail(CPECAN_EINVAL, "batch was not created with CPECAN_FLAG_DEBUG_DUMP");
    const DevItem &d = b->hItems[(size_t) item];
    if (nCells < d.nCells) return fail(CPECAN_EOVERFLOW, "need room for %lld cells", d.nCells);
    HIP_TRY(hipSetDevice(b->ctx->device));
    if (b->ran) HIP_TRY(hipEventSynchronize(b->ev2));
    if (forward)
        HIP_TRY(hipMemcpy(forward, b->Fstore.p + d.cellBase * 3, (size_t) d.nCells * 3 * sizeof(double),
                          hipMemcpyDeviceToHost));
    if (backward)
        HIP_TRY(hipMemcpy(backward, b->dbgB.p + d.cellBase * 3, (size_t) d.nCells * 3 * sizeof(double),
                          hipMemcpyDeviceToHost));
    return CPECAN_OK;
}

} /* extern "C" */
