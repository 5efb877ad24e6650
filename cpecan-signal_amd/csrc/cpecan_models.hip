/*
 * cpecan_models.hip -- the model tables of a context (ModelTable, cpecan_ctx.h): the host-libm derivation of every
 * machine's device block, the create, download and in-place update calls of include/cpecan_hip.h, and the four small
 * kernels that assemble or rewrite tables on the device.
 */
#include "cpecan_ctx.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <memory>
#include <thread>

/* One derived row per k-mer.  K = log_inv_sqrt_2pi - log(sigma) is the part of
 * emissions_signal_logGaussPdf (impl/stateMachine.c:333-343) that does not depend on the event;
 * evaluated here with the host libm exactly as the reference's per-cell code would. */
static void derive_rows(const cpecan_sm3_model *m, double *dst) {
    const double c = -0.91893853320467267;
    for (int i = 0; i < 9; i++) dst[i] = m->transitions[i];
    for (int i = 9; i < CP_MODEL_HEADER; i++) dst[i] = 0.0;
    double *rows = dst + CP_MODEL_HEADER;
    for (int k = 0; k <= CPECAN_NUM_KMERS; k++) {
        double *r = rows + (size_t) k * CP_ROW;
        if (k == CPECAN_NUM_KMERS) { /* "not a k-mer": model reads 0.0, gap prob LOG_ZERO (:185,:223) */
            for (int j = 0; j < CP_ROW; j++) r[j] = 0.0;
            r[CP_K1] = r[CP_K2] = r[CP_YK1] = r[CP_YK2] = -INFINITY;
            r[CP_GAPX] = -INFINITY;
            continue;
        }
        const double *a = m->match_probs + 1 + (size_t) k * CPECAN_MODEL_PARAMS;
        const double *b = m->gap_y_probs + 1 + (size_t) k * CPECAN_MODEL_PARAMS;
        const double sd[4] = { a[1], a[3], b[1], b[3] };
        const double mu[4] = { a[0], a[2], b[0], b[2] };
        for (int g = 0; g < 4; g++) {
            double *q = r + 4 * g;
            q[0] = mu[g];
            q[1] = sd[g];
            q[2] = sd[g] == 0.0 ? 0.0 : 1.0 / sd[g];
            q[3] = sd[g] == 0.0 ? -INFINITY : c - log(sd[g]);
        }
        r[CP_GAPX] = m->gap_x_probs[k];
        r[17] = 0.0;
    }
}

int ModelTable::grow(cpecan_ctx *c, int32_t more, double **fresh) {
    const size_t old = (size_t) n * stride, total = old + (size_t) more * stride;
    (void) ctx_fence(c); /* (the old table goes back to the allocator's cache) */
    DevBuf<double> grown;
    hipError_t e = grown.alloc(total);
    if (e != hipSuccess) return fail(CPECAN_EHIP, "model table allocation: %s", hipGetErrorString(e));
    {
        StreamFence fence{ c->prep, nullptr };
        /* on the stream the uploads that follow use, and over before the old block is released */
        if (old) HIP_TRY(hipMemcpyAsync(grown.p, block.p, old * sizeof(double), hipMemcpyDeviceToDevice, c->prep));
    }
    grown.swap(block);
    *fresh = block.p + old;
    return CPECAN_OK;
}

/* an upload into the grown table went wrong (e, or the runtime's last error): the second half of ModelTable's failure
 * rule.  The prep stream is idle and grow() has waited for the table's readers. */
static int table_lost(cpecan_ctx *c, ModelTable &t, hipError_t e) {
    t.drop();
    c->modelEpoch++;
    return fail(CPECAN_EHIP, "model table upload failed: %s", hipGetErrorString(e != hipSuccess ? e : hipGetLastError()));
}

static int pool_threads(int32_t threads, int32_t n) {
    const int nt = threads > 0 ? threads : host_threads();
    return std::max(1, std::min(nt, (int) n));
}

/* n models derived by nt host threads while they upload: every thread derives up to `per` neighbouring models into one
 * of its two pinned slots (derive(i, dst): model i of the call) and sends the slot on its way; the slot is written
 * again once its copy has gone, so no host copy of the whole table exists at any time.  `derived`: the lap's label. */
template <class Derive>
static int create_threaded(cpecan_ctx *c, Machine machine, Lap &lap, const char *derived, int32_t n, int nt, int per,
                           Derive derive, const double *side, int32_t *ids) {
    ModelTable &t = c->tables[machine];
    const size_t blockBytes = t.stride * sizeof(double), slotBytes = blockBytes * (size_t) per;
    int rc = pinned_slots(c, slotBytes * 2 * (size_t) nt);
    if (rc != CPECAN_OK) return rc;
    /* one event per slot, made before the table grows and destroyed whichever way the call returns */
    struct Events {
        std::vector<hipEvent_t> ev;
        ~Events() {
            for (hipEvent_t e : ev)
                if (e) (void) hipEventDestroy(e);
        }
    } gone{ std::vector<hipEvent_t>(2 * (size_t) nt, nullptr) };
    for (auto &ev : gone.ev) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    double *fresh = nullptr;
    rc = t.grow(c, n, &fresh);
    if (rc != CPECAN_OK) return rc;
    lap("device table, pinned slots");
    std::atomic<int> bad{0};
    std::vector<std::thread> pool;
    for (int w = 0; w < nt; w++)
        pool.emplace_back([&, w]() {
            if (hipSetDevice(c->device) != hipSuccess) { bad = 1; return; }
            int turn = 0;
            for (int i = w * per; i < n; i += nt * per, turn++) {
                const size_t slot = 2 * (size_t) w + (turn & 1);
                double *dst = (double *) ((char *) c->pinned + slot * slotBytes);
                const int m = std::min(per, (int) n - i); /* models of this slot */
                if (turn >= 2 && hipEventSynchronize(gone.ev[slot]) != hipSuccess) { bad = 1; return; }
                for (int j = 0; j < m; j++) derive(i + j, dst + (size_t) j * t.stride);
                if (hipMemcpyAsync(fresh + (size_t) i * t.stride, dst, blockBytes * (size_t) m, hipMemcpyHostToDevice, c->prep) != hipSuccess ||
                    hipEventRecord(gone.ev[slot], c->prep) != hipSuccess) { bad = 1; return; }
            }
        });
    for (auto &th : pool) th.join();
    const hipError_t se = hipStreamSynchronize(c->prep);
    if (bad || se != hipSuccess) return table_lost(c, t, se);
    lap(derived);
    t.commit(n, side, ids);
    return CPECAN_OK;
}

static int download(cpecan_ctx *c, Machine machine, const char *whose, int32_t id, double *out, int64_t capacity,
                    int64_t *nDoubles) {
    if (!c || !nDoubles) return fail(CPECAN_EINVAL, "bad argument");
    const ModelTable &t = c->tables[machine];
    *nDoubles = (int64_t) t.stride;
    if (!out) return CPECAN_OK;
    if (id < 0 || id >= t.n) return fail(CPECAN_EINVAL, "%smodel id %d out of range (%d)", whose, id, t.n);
    if (capacity < (int64_t) t.stride) return fail(CPECAN_EINVAL, "capacity %lld < %d doubles", (long long) capacity, (int) t.stride);
    HIP_TRY(hipSetDevice(c->device));
    MemScope mem(c->mem);
    HIP_TRY(ctx_fence(c));
    HIP_TRY(hipMemcpy(out, t.block.p + (size_t) id * t.stride, t.stride * sizeof(double), hipMemcpyDeviceToHost));
    return CPECAN_OK;
}

int cpecan_hip_models_create(cpecan_ctx *c, const cpecan_sm3_model *models, int32_t n,
                             int32_t threads, int32_t *ids) {
    if (!c || !models || n <= 0 || !ids) return fail(CPECAN_EINVAL, "bad argument");
    for (int i = 0; i < n; i++)
        if (!models[i].match_probs || !models[i].gap_x_probs || !models[i].gap_y_probs)
            return fail(CPECAN_EINVAL, "model %d has a NULL table", i);
    HIP_TRY(hipSetDevice(c->device));
    MemScope mem(c->mem);
    Lap lap("models_create");
    std::vector<double> switchToX((size_t) n);
    for (int i = 0; i < n; i++) switchToX[(size_t) i] = models[i].transitions[T_GAP_SWITCH_TO_X];
    return create_threaded(c, STRAWMAN, lap, "derive rows (threads) || upload", n, pool_threads(threads, n), 1,
                           [&](int i, double *dst) { derive_rows(&models[i], dst); }, switchToX.data(), ids);
}

/* One element of one read's derived table from the base model's derived table, the read's scaling parameters
 * (emissions_signal_scaleModel impl/stateMachine.c:631-651) and the three values per k-mer the host took with its
 * libm (K1, the scaled noise sd, K2): every other entry is one IEEE multiply, add or divide, rounded as on the host. */
extern "C" __global__ void cpecan_k_scale_models(const double *base, const double *scalings /* n x 5 */,
                                                 const double *hostPart /* n x 4096 x 3 */, int n, double *out) {
    const long long e = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= CP_MODEL_STRIDE) return;
    const double b = base[e];
    const long long r = e - CP_MODEL_HEADER;
    const int k = r >= 0 ? (int) (r / CP_ROW) : -1, j = r >= 0 ? (int) (r % CP_ROW) : -1;
    const bool plain = k < 0 || k >= CPECAN_NUM_KMERS || j >= 8;
    /* the neighbours a derived entry needs: the level sd (j 1, 2), the noise mean's row mates */
    const double sd = plain ? 0.0 : base[CP_MODEL_HEADER + (long long) k * CP_ROW + 1];
    for (int m = blockIdx.y; m < n; m += gridDim.y) {
        double v = b;
        if (!plain) {
            const double *sc = scalings + 5 * (long long) m;
            const double *h = hostPart + ((long long) m * CPECAN_NUM_KMERS + k) * 3;
            switch (j) {
            case 0: v = __dadd_rn(__dmul_rn(b, sc[0]), sc[1]); break;
            case 1: v = __dmul_rn(b, sc[2]); break;
            case 2: { const double s = __dmul_rn(sd, sc[2]); v = s == 0.0 ? 0.0 : __ddiv_rn(1.0, s); break; }
            case 3: v = h[0]; break;
            case 4: v = __dmul_rn(b, sc[3]); break;
            case 5: v = h[1]; break;
            case 6: v = h[1] == 0.0 ? 0.0 : __ddiv_rn(1.0, h[1]); break;
            default: v = h[2]; break;
            }
        }
        out[(long long) m * CP_MODEL_STRIDE + e] = v;
    }
}

/* n models of one base model, one per read's scaling parameters, assembled on the device: the host threads take what
 * needs the host libm (hostPart(scaling, dst): partDoubles values of one read), the kernel behind launch(base, scalings,
 * part, out) writes the blocks from the base model's block, the scalings and those values. */
template <class HostPart, class Launch>
static int create_scaled(cpecan_ctx *c, Machine machine, Lap &lap, const std::vector<double> &baseBlock,
                         const cpecan_read_scaling *scalings, int32_t n, int32_t threads, size_t partDoubles,
                         HostPart hostPart, Launch launch, double sideValue, int32_t *ids) {
    ModelTable &t = c->tables[machine];
    PinnedBuf<double> part; /* (recycled pinned memory: no page faults, and the copy engine reads it directly) */
    HIP_TRY(part.alloc((size_t) n * partDoubles));
    const int nt = pool_threads(threads, n);
    std::vector<std::thread> pool;
    for (int w = 0; w < nt; w++)
        pool.emplace_back([&, w]() {
            for (int i = w; i < n; i += nt) hostPart(scalings[i], part.p + (size_t) i * partDoubles);
        });
    for (auto &th : pool) th.join();
    lap("host libm part (threads)");
    DevBuf<double> dBase, dScal, dPart;
    StreamFence fence{ c->prep, nullptr };
    HIP_TRY(dBase.alloc(baseBlock.size()));
    HIP_TRY(dScal.alloc((size_t) n * 5));
    HIP_TRY(dPart.alloc(part.n));
    double *fresh = nullptr;
    const int rc = t.grow(c, n, &fresh);
    if (rc != CPECAN_OK) return rc;
    lap("device table");
    static_assert(sizeof(cpecan_read_scaling) == 5 * sizeof(double), "cpecan_read_scaling is five doubles");
    hipError_t e = hipMemcpyAsync(dBase.p, baseBlock.data(), baseBlock.size() * sizeof(double), hipMemcpyHostToDevice, c->prep);
    if (e == hipSuccess) e = hipMemcpyAsync(dScal.p, scalings, (size_t) n * 5 * sizeof(double), hipMemcpyHostToDevice, c->prep);
    if (e == hipSuccess) e = hipMemcpyAsync(dPart.p, part.p, part.n * sizeof(double), hipMemcpyHostToDevice, c->prep);
    if (e == hipSuccess) {
        launch((const double *) dBase.p, (const double *) dScal.p, (const double *) dPart.p, fresh);
        e = hipGetLastError();
    }
    const hipError_t se = hipStreamSynchronize(c->prep); /* the staging blocks are released on return */
    if (e != hipSuccess || se != hipSuccess) return table_lost(c, t, e != hipSuccess ? e : se);
    lap("upload + assemble");
    const std::vector<double> side((size_t) n, sideValue);
    t.commit(n, side.data(), ids);
    return CPECAN_OK;
}

int cpecan_hip_models_create_scaled(cpecan_ctx *c, const cpecan_sm3_model *base, const cpecan_read_scaling *scalings,
                                    int32_t n, int32_t threads, int32_t *ids) {
    if (!c || !base || !scalings || n <= 0 || !ids) return fail(CPECAN_EINVAL, "bad argument");
    if (!base->match_probs || !base->gap_x_probs || !base->gap_y_probs) return fail(CPECAN_EINVAL, "the base model has a NULL table");
    HIP_TRY(hipSetDevice(c->device));
    MemScope mem(c->mem);
    Lap lap("models_create_scaled");
    std::vector<double> baseRows(CP_MODEL_STRIDE);
    derive_rows(base, baseRows.data());
    return create_scaled(
        c, STRAWMAN, lap, baseRows, scalings, n, threads, (size_t) CPECAN_NUM_KMERS * 3,
        [&](const cpecan_read_scaling &s, double *dst) {
            const double lg = -0.91893853320467267;
            for (int k = 0; k < CPECAN_NUM_KMERS; k++) {
                const double *a = base->match_probs + 1 + (size_t) k * CPECAN_MODEL_PARAMS;
                const double sd = a[1] * s.var;
                const double nmu = a[2] * s.scale_sd, lambda = a[4] * s.var_sd;
                const double nsd = sqrt(pow(nmu, 3.0) / lambda);
                dst[3 * k] = sd == 0.0 ? -INFINITY : lg - log(sd);
                dst[3 * k + 1] = nsd;
                dst[3 * k + 2] = nsd == 0.0 ? -INFINITY : lg - log(nsd);
            }
        },
        [&](const double *dBase, const double *dScal, const double *dPart, double *out) {
            hipLaunchKernelGGL(cpecan_k_scale_models, dim3((unsigned) ((CP_MODEL_STRIDE + 255) / 256), (unsigned) std::min(n, 65535)),
                               dim3(256), 0, c->prep, dBase, dScal, dPart, (int) n, out);
        },
        base->transitions[T_GAP_SWITCH_TO_X], ids);
}

int cpecan_hip_models_download(cpecan_ctx *c, int32_t id, double *out, int64_t capacity, int64_t *nDoubles) {
    return download(c, STRAWMAN, "", id, out, capacity, nDoubles);
}

extern "C" __global__ void cpecan_k_set_transitions(double *models, int nModels, const double *values /* 9 + 4096 */,
                                                    int withGap) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    for (int m = blockIdx.y; m < nModels; m += gridDim.y) { /* grid.y is capped at 65535 */
        double *blk = models + (long long) m * CP_MODEL_STRIDE;
        if (i < 9) blk[i] = values[i];
        else if (withGap && i < 9 + CPECAN_NUM_KMERS)
            blk[CP_MODEL_HEADER + (long long) (i - 9) * CP_ROW + CP_GAPX] = values[i];
    }
}

int cpecan_hip_models_set_transitions(cpecan_ctx *c, const double *transitions, const double *gapX) {
    if (!c || !transitions) return fail(CPECAN_EINVAL, "bad argument");
    ModelTable &t = c->tables[STRAWMAN];
    if (t.n <= 0) return fail(CPECAN_EINVAL, "the context holds no strawMan models");
    HIP_TRY(hipSetDevice(c->device));
    MemScope mem(c->mem);
    std::vector<double> v(9 + CPECAN_NUM_KMERS, 0.0);
    for (int i = 0; i < 9; i++) v[(size_t) i] = transitions[i];
    if (gapX) std::copy(gapX, gapX + CPECAN_NUM_KMERS, v.begin() + 9);
    for (double &s : t.side) s = transitions[T_GAP_SWITCH_TO_X];
    /* the tables are written in place: every run that reads them is over first (on whatever lanes it went); the
     * update goes through the context's own prep stream, which no other context's run shares */
    HIP_TRY(ctx_fence(c));
    DevBuf<double> dv;
    StreamFence fence{ c->prep, nullptr };
    HIP_TRY(dv.alloc(v.size()));
    HIP_TRY(hipMemcpyAsync(dv.p, v.data(), v.size() * sizeof(double), hipMemcpyHostToDevice, c->prep));
    hipLaunchKernelGGL(cpecan_k_set_transitions, dim3((9 + CPECAN_NUM_KMERS + 255) / 256, (unsigned) std::min(t.n, 65535)),
                       dim3(256), 0, c->prep, t.block.p, t.n, (const double *) dv.p, gapX ? 1 : 0);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->prep)); /* dv is released on return */
    return CPECAN_OK;
}

/* Device block of one vanilla model.  Every log() the reference takes per cell
 * (stateMachine3Vanilla_cellCalculate :1391-1407, logGaussPdf :338, logInvGaussPdf :328) depends on the
 * skip bin or the k-mer only: taken here once, with the host libm the reference would call. */
static void derive_vanilla_bins(double m_to_y_not_x, const double *skip_probs, double *bins /* 30 x 5 */) {
    for (int bin = 0; bin < 30; bin++) {
        const double a_mx = skip_probs[bin];
        const double a_my = (1 - a_mx) * m_to_y_not_x;
        const double a_mm = 1.0f - a_my - a_mx;
        const double a_xx = skip_probs[bin + 30];
        const double a_xm = 1.0f - a_xx;
        double *b = bins + bin * 5;
        b[0] = log(a_mx);
        b[1] = log(a_xx);
        b[2] = log(a_mm);
        b[3] = log(a_xm);
        b[4] = log(a_my);
    }
}

static void derive_vanilla(const cpecan_vanilla_model *m, double *dst, bool echelon = false) {
    for (int i = 0; i < CP_VHDR; i++) dst[i] = 0.0;
    dst[0] = m->m_to_y_not_x;
    dst[1] = m->e_to_e;
    dst[CP_VHDR_END_M] = m->end_match_prob;
    dst[CP_VHDR_END_X] = m->end_from_x_prob;
    dst[CP_VHDR_END_Y] = m->end_from_y_prob;
    const double a_yy = m->e_to_e, a_ym = 1.0f - a_yy;
    dst[CP_VHDR_LOG_YY] = log(a_yy);
    dst[CP_VHDR_LOG_YM] = log(a_ym);
    derive_vanilla_bins(m->m_to_y_not_x, m->skip_probs, dst + CP_VHDR_BINS);
    const double c = -0.91893853320467267;
    double *rows = dst + CP_VHDR;
    for (int k = 0; k <= CPECAN_NUM_KMERS; k++) {
        double *r = rows + (size_t) k * CP_VROW;
        for (int t = 0; t < 2; t++) {
            double *q = r + 6 * t;
            if (k == CPECAN_NUM_KMERS) {
                /* not a k-mer: the reference's model accessors read 0.0 for an index past the table (:221-240), so the
                 * level term is LOG_ZERO (sd 0) and the noise term NaN (mean 0, lambda 0: 0 * inf), and their sum, the
                 * emission, NaN -- reproduced here; the echelon machine keeps its noise term finite (its host DP's) */
                q[CP_V_MU] = 0.0; q[CP_V_SD] = 0.0; q[CP_V_K] = -INFINITY;
                q[CP_V_NMU] = echelon ? 1.0 : 0.0; q[CP_V_LAMBDA] = echelon ? 1.0 : 0.0;
                q[CP_V_LLAMBDA] = echelon ? 0.0 : -INFINITY;
                continue;
            }
            const double *a = (t ? m->gap_y_probs : m->match_probs) + 1 + (size_t) k * CPECAN_MODEL_PARAMS;
            q[CP_V_MU] = a[0];
            q[CP_V_SD] = a[1];
            q[CP_V_K] = a[1] == 0.0 ? -INFINITY : c - log(a[1]);
            q[CP_V_NMU] = a[2];
            q[CP_V_LAMBDA] = a[4];
            q[CP_V_LLAMBDA] = log(a[4]);
        }
    }
}

int cpecan_hip_modelsv_create(cpecan_ctx *c, const cpecan_vanilla_model *models, int32_t n, int32_t threads,
                              int32_t *ids) {
    if (!c || !models || n <= 0 || !ids) return fail(CPECAN_EINVAL, "bad argument");
    for (int i = 0; i < n; i++)
        if (!models[i].match_probs || !models[i].skip_probs || !models[i].gap_y_probs)
            return fail(CPECAN_EINVAL, "model %d has a NULL table", i);
    HIP_TRY(hipSetDevice(c->device));
    MemScope mem(c->mem);
    Lap lap("modelsv_create");
    const int nt = pool_threads(threads, n);
    /* a slot holds up to four neighbouring models: the copy engine's cost per copy is that of a block's transfer, so
     * one copy per model would double the upload */
    const int per = std::max(1, std::min(4, (int) n / (2 * nt)));
    std::vector<double> mToY((size_t) n);
    for (int i = 0; i < n; i++) mToY[(size_t) i] = models[i].m_to_y_not_x;
    return create_threaded(c, VANILLA, lap, "derive blocks (threads) || upload", n, nt, per,
                           [&](int i, double *dst) { derive_vanilla(&models[i], dst); }, mToY.data(), ids);
}

/* Two neighbouring elements of one read's vanilla block from the base model's block, the read's scaling parameters
 * (emissions_signal_scaleModel impl/stateMachine.c:631-651, which rewrites the match table only) and the two values
 * per k-mer the host took with its libm (K and log lambda of the scaled match row): header, the extra-event half of
 * every row and the "not a k-mer" row are the base's; every other entry is one IEEE multiply or add, rounded as on the
 * host.  An element pair never straddles a row half (header, row and half are even), and a block starts on 16 bytes. */
extern "C" __global__ void cpecan_k_scale_models_v(const double *base, const double *scalings /* n x 5 */,
                                                   const double *hostPart /* n x 4096 x 2 */, int n, double *out) {
    const long long e = 2 * ((long long) blockIdx.x * blockDim.x + threadIdx.x);
    if (e >= CP_VMODEL_STRIDE) return;
    const double2 b = *(const double2 *) (base + e);
    const long long r = e - CP_VHDR;
    const int k = r >= 0 ? (int) (r / CP_VROW) : -1, j = r >= 0 ? (int) (r % CP_VROW) : -1;
    const bool plain = k < 0 || k >= CPECAN_NUM_KMERS || j >= 6;
    for (int m = blockIdx.y; m < n; m += gridDim.y) {
        double2 v = b;
        if (!plain) {
            const double *sc = scalings + 5 * (long long) m;
            const double *h = hostPart + ((long long) m * CPECAN_NUM_KMERS + k) * 2;
            if (j == CP_V_MU) { /* level mean, level sd */
                v.x = __dadd_rn(__dmul_rn(b.x, sc[0]), sc[1]);
                v.y = __dmul_rn(b.y, sc[2]);
            } else if (j == CP_V_K) { /* K, noise mean */
                v.x = h[0];
                v.y = __dmul_rn(b.y, sc[3]);
            } else { /* noise lambda and its log */
                v.x = __dmul_rn(b.x, sc[4]);
                v.y = h[1];
            }
        }
        *(double2 *) (out + (long long) m * CP_VMODEL_STRIDE + e) = v;
    }
}

int cpecan_hip_modelsv_create_scaled(cpecan_ctx *c, const cpecan_vanilla_model *base, const cpecan_read_scaling *scalings,
                                     int32_t n, int32_t threads, int32_t *ids) {
    if (!c || !base || !scalings || n <= 0 || !ids) return fail(CPECAN_EINVAL, "bad argument");
    if (!base->match_probs || !base->skip_probs || !base->gap_y_probs) return fail(CPECAN_EINVAL, "the base model has a NULL table");
    HIP_TRY(hipSetDevice(c->device));
    MemScope mem(c->mem);
    Lap lap("modelsv_create_scaled");
    static_assert(CP_VHDR % 2 == 0 && CP_VROW % 2 == 0 && CP_V_MU == 0 && CP_V_K == 2 && CP_V_LAMBDA == 4,
                  "cpecan_k_scale_models_v writes a block as pairs of doubles");
    std::vector<double> baseBlock(CP_VMODEL_STRIDE);
    derive_vanilla(base, baseBlock.data());
    return create_scaled(
        c, VANILLA, lap, baseBlock, scalings, n, threads, (size_t) CPECAN_NUM_KMERS * 2,
        [&](const cpecan_read_scaling &s, double *dst) {
            const double lg = -0.91893853320467267;
            for (int k = 0; k < CPECAN_NUM_KMERS; k++) { /* what derive_vanilla takes of the scaled match row */
                const double *a = base->match_probs + 1 + (size_t) k * CPECAN_MODEL_PARAMS;
                const double sd = a[1] * s.var, lambda = a[4] * s.var_sd;
                dst[2 * k] = sd == 0.0 ? -INFINITY : lg - log(sd);
                dst[2 * k + 1] = log(lambda);
            }
        },
        [&](const double *dBase, const double *dScal, const double *dPart, double *out) {
            hipLaunchKernelGGL(cpecan_k_scale_models_v, dim3((unsigned) ((CP_VMODEL_STRIDE / 2 + 255) / 256), (unsigned) std::min(n, 65535)),
                               dim3(256), 0, c->prep, dBase, dScal, dPart, (int) n, out);
        },
        base->m_to_y_not_x, ids);
}

int cpecan_hip_modelsv_download(cpecan_ctx *c, int32_t id, double *out, int64_t capacity, int64_t *nDoubles) {
    return download(c, VANILLA, "vanilla ", id, out, capacity, nDoubles);
}

/* every vanilla model receives the 150 logs of the set whose fudge factor is its own (header entry 0, compared as bits) */
extern "C" __global__ void cpecan_k_set_skip_bins(double *models, int nModels, const double *factors, int nSets,
                                                  const double *bins /* nSets x 150 */) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 150) return;
    for (int m = blockIdx.y; m < nModels; m += gridDim.y) { /* grid.y is capped at 65535 */
        double *blk = models + (long long) m * CP_VMODEL_STRIDE;
        const long long mine = __double_as_longlong(blk[0]);
        for (int s = 0; s < nSets; s++)
            if (__double_as_longlong(factors[s]) == mine) {
                blk[CP_VHDR_BINS + i] = bins[s * 150 + i];
                break;
            }
    }
}

int cpecan_hip_modelsv_set_skip_probs(cpecan_ctx *c, const double *skipProbs) {
    if (!c || !skipProbs) return fail(CPECAN_EINVAL, "bad argument");
    ModelTable &t = c->tables[VANILLA];
    if (t.n <= 0) return fail(CPECAN_EINVAL, "the context holds no vanilla models");
    HIP_TRY(hipSetDevice(c->device));
    MemScope mem(c->mem);
    /* log a_my and log a_mm depend on the model's m_to_y_not_x: one set of 150 logs per distinct value, taken by the
     * code derive_vanilla runs */
    std::vector<double> v; /* [factors: nSets | bins: nSets x 150] once the sets are known */
    std::vector<double> factors;
    for (double f : t.side) {
        bool seen = false;
        for (double g : factors) seen = seen || memcmp(&f, &g, sizeof f) == 0;
        if (!seen) factors.push_back(f);
    }
    const size_t nSets = factors.size();
    v.assign(nSets * 151, 0.0);
    for (size_t s = 0; s < nSets; s++) {
        v[s] = factors[s];
        derive_vanilla_bins(factors[s], skipProbs, v.data() + nSets + s * 150);
    }
    /* the tables are written in place: every run that reads them is over first (on whatever lanes it went); the
     * update goes through the context's own prep stream, which no other context's run shares */
    HIP_TRY(ctx_fence(c));
    DevBuf<double> dv;
    StreamFence fence{ c->prep, nullptr };
    HIP_TRY(dv.alloc(v.size()));
    HIP_TRY(hipMemcpyAsync(dv.p, v.data(), v.size() * sizeof(double), hipMemcpyHostToDevice, c->prep));
    hipLaunchKernelGGL(cpecan_k_set_skip_bins, dim3(1, (unsigned) std::min(t.n, 65535)), dim3(192), 0, c->prep,
                       t.block.p, t.n, (const double *) dv.p, (int) nSets, (const double *) (dv.p + nSets));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->prep)); /* dv is released on return */
    return CPECAN_OK;
}

/* Device block of one echelon model: the vanilla layout (rows, end values) with the machine's own per-bin logs
 * (stateMachineEchelon_cellCalculate :1418-1425: log beta, log alpha, log(1 - beta), log(1 - alpha)) and log(n) of
 * emissions_signal_multipleKmerMatchProb (:548), all taken with the host libm. */
static void derive_echelon(const cpecan_echelon_model *m, double *dst) {
    cpecan_vanilla_model v = {};
    v.end_match_prob = m->end_match_prob;
    v.end_from_x_prob = m->end_from_x_prob;
    v.match_probs = m->match_probs;
    v.skip_probs = m->skip_probs;
    v.gap_y_probs = m->gap_y_probs;
    derive_vanilla(&v, dst, true);
    for (int i = 0; i < CP_VHDR; i++) dst[i] = 0.0;
    dst[CP_VHDR_END_M] = m->end_match_prob;
    dst[CP_VHDR_END_X] = m->end_from_x_prob;
    for (int bin = 0; bin < 30; bin++) {
        const double a_mx = m->skip_probs[bin], a_mh = 1 - a_mx;
        const double a_xx = m->skip_probs[bin + 30], a_xh = 1 - a_xx;
        double *b = dst + CP_VHDR_BINS + bin * 5;
        b[0] = log(a_mx);
        b[1] = log(a_xx);
        b[2] = log(a_mh);
        b[3] = log(a_xh);
        b[4] = 0.0;
    }
    for (int n = 0; n < 8; n++) dst[CP_EMODEL_LOGN + n] = n >= 1 && n <= 5 ? log((double) n) : 0.0;
}

/* The creates of a handful of models per call (echelon, HDP descriptors, 5-state, 4-state): the new rows, derived on
 * the host, go to the end of the grown table in one copy.  side: a value per model, or null where the host needs none. */
static int append_rows(cpecan_ctx *c, Machine machine, const std::vector<double> &rows, int32_t n, const double *side,
                       int32_t *ids) {
    ModelTable &t = c->tables[machine];
    double *fresh = nullptr;
    const int rc = t.grow(c, n, &fresh);
    if (rc != CPECAN_OK) return rc;
    const hipError_t e = hipMemcpyAsync(fresh, rows.data(), rows.size() * sizeof(double), hipMemcpyHostToDevice, c->prep);
    const hipError_t se = hipStreamSynchronize(c->prep);
    if (e != hipSuccess || se != hipSuccess) return table_lost(c, t, e != hipSuccess ? e : se);
    const std::vector<double> none((size_t) n, 0.0);
    t.commit(n, side ? side : none.data(), ids);
    return CPECAN_OK;
}

int cpecan_hip_modelse_create(cpecan_ctx *c, const cpecan_echelon_model *models, int32_t n, int32_t *ids) {
    if (!c || !models || n <= 0 || !ids) return fail(CPECAN_EINVAL, "bad argument");
    for (int i = 0; i < n; i++)
        if (!models[i].match_probs || !models[i].skip_probs || !models[i].gap_y_probs)
            return fail(CPECAN_EINVAL, "model %d has a NULL table", i);
    HIP_TRY(hipSetDevice(c->device));
    MemScope mem(c->mem);
    std::vector<double> rows((size_t) n * CP_EMODEL_STRIDE);
    for (int i = 0; i < n; i++) derive_echelon(&models[i], rows.data() + (size_t) i * CP_EMODEL_STRIDE);
    return append_rows(c, ECHELON, rows, n, nullptr, ids);
}

/* the tables the HDP descriptors point to go with the descriptors */
static void hdp_tables_release(cpecan_ctx *c) {
    for (auto *t : c->hdpTables) delete t;
    c->hdpTables.clear();
    c->hdpAlphabet.clear();
}

int cpecan_hip_modelsh_create(cpecan_ctx *c, const cpecan_hdp_model *models, int32_t n, int32_t *ids) {
    if (!c || !models || n <= 0 || !ids) return fail(CPECAN_EINVAL, "bad argument");
    std::string alphabet = c->hdpAlphabet; /* the context's once the call has gone through */
    for (int i = 0; i < n; i++) {
        const cpecan_hdp_model &m = models[i];
        if (!m.alphabet || m.alphabet_size < 1 || m.alphabet_size > 16 || m.grid_length < 2 || !m.grid ||
            m.n_rows < 1 || !m.posterior_predictive || !m.spline_slopes || !m.kmer_row)
            return fail(CPECAN_EINVAL, "HDP model %d is incomplete", i);
        /* the register-resident kernels carry a table row's offset (row x grid_length, in doubles) as a 32-bit index */
        if ((long long) m.n_rows * m.grid_length > 0xffffffffLL)
            return fail(CPECAN_EINVAL, "HDP model %d: tables of more than 2^32 - 1 values", i);
        const std::string a(m.alphabet, (size_t) m.alphabet_size);
        if (!alphabet.empty() && alphabet != a)
            return fail(CPECAN_EINVAL, "all HDP models of a context must share one alphabet");
        alphabet = a;
        long long nK = 1;
        for (int q = 0; q < 6; q++) nK *= m.alphabet_size;
        for (long long k = 0; k < nK; k++)
            if (m.kmer_row[k] < 0 || m.kmer_row[k] >= m.n_rows)
                return fail(CPECAN_EINVAL, "HDP model %d: k-mer %lld points outside the tables", i, k);
    }
    HIP_TRY(hipSetDevice(c->device));
    MemScope mem(c->mem);
    /* every model's tables are on the device before anything of the call is committed, and go back to the allocator
     * if the call fails: a failed call leaves none of its models behind */
    std::vector<std::unique_ptr<cpecan_ctx::HdpTables>> tables;
    std::vector<double> rows((size_t) n * CP_HDP_MODEL_DOUBLES), switchToX((size_t) n);
    for (int i = 0; i < n; i++) {
        const cpecan_hdp_model &m = models[i];
        long long nK = 1;
        for (int q = 0; q < 6; q++) nK *= m.alphabet_size;
        tables.emplace_back(new cpecan_ctx::HdpTables());
        cpecan_ctx::HdpTables *t = tables.back().get();
        const size_t cells = (size_t) m.n_rows * (size_t) m.grid_length;
        HIP_TRY(t->kmerRow.alloc((size_t) nK));
        HIP_TRY(t->grid.alloc((size_t) m.grid_length));
        HIP_TRY(t->y.alloc(cells));
        HIP_TRY(t->slope.alloc(cells));
        HIP_TRY(hipMemcpy(t->kmerRow.p, m.kmer_row, (size_t) nK * sizeof(int), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(t->grid.p, m.grid, (size_t) m.grid_length * sizeof(double), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(t->y.p, m.posterior_predictive, cells * sizeof(double), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(t->slope.p, m.spline_slopes, cells * sizeof(double), hipMemcpyHostToDevice));
        DevHdpModel d;
        for (int q = 0; q < 9; q++) d.t[q] = m.transitions[q];
        d.gridLength = m.grid_length;
        d.pad = 0;
        d.kmerRow = t->kmerRow.p;
        d.grid = t->grid.p;
        d.y = t->y.p;
        d.slope = t->slope.p;
        memcpy(rows.data() + (size_t) i * CP_HDP_MODEL_DOUBLES, &d, sizeof d);
        switchToX[(size_t) i] = d.t[T_GAP_SWITCH_TO_X];
    }
    const int rc = append_rows(c, HDP, rows, n, switchToX.data(), ids);
    if (rc != CPECAN_OK) {
        if (c->tables[HDP].n == 0) hdp_tables_release(c); /* (the descriptors were dropped, or there were none) */
        return rc;
    }
    for (auto &t : tables) c->hdpTables.push_back(t.release());
    c->hdpAlphabet = alphabet;
    return CPECAN_OK;
}

int cpecan_hip_models5_create(cpecan_ctx *c, const cpecan_sm5_model *models, int32_t n, int32_t *ids) {
    if (!c || !models || n <= 0 || !ids) return fail(CPECAN_EINVAL, "bad argument");
    HIP_TRY(hipSetDevice(c->device));
    MemScope mem(c->mem);
    std::vector<double> rows((size_t) n * CP_MODEL5_STRIDE, 0.0);
    for (int i = 0; i < n; i++) {
        double *m = rows.data() + (size_t) i * CP_MODEL5_STRIDE;
        for (int k = 0; k < 17; k++) m[k] = models[i].transitions[k];
        for (int k = 0; k < 16; k++) m[24 + k] = models[i].match_probs[k];
        for (int k = 0; k < 4; k++) m[40 + k] = models[i].gap_x_probs[k];
        for (int k = 0; k < 4; k++) m[44 + k] = models[i].gap_y_probs[k];
    }
    return append_rows(c, DNA5, rows, n, nullptr, ids);
}

/* 4-state signal models (getStateMachine4): the strawMan rows with the machine's eleven transitions in the header */
int cpecan_hip_models4_create(cpecan_ctx *c, const cpecan_sm4_model *models, int32_t n, int32_t *ids) {
    if (!c || !models || n <= 0 || !ids) return fail(CPECAN_EINVAL, "bad argument");
    for (int i = 0; i < n; i++)
        if (!models[i].match_probs || !models[i].gap_x_probs || !models[i].gap_y_probs)
            return fail(CPECAN_EINVAL, "model %d has a NULL table", i);
    HIP_TRY(hipSetDevice(c->device));
    MemScope mem(c->mem);
    std::vector<double> rows((size_t) n * CP_MODEL_STRIDE);
    for (int i = 0; i < n; i++) {
        cpecan_sm3_model m3;
        for (int k = 0; k < 9; k++) m3.transitions[k] = models[i].transitions[k];
        m3.match_probs = models[i].match_probs;
        m3.gap_x_probs = models[i].gap_x_probs;
        m3.gap_y_probs = models[i].gap_y_probs;
        double *dst = rows.data() + (size_t) i * CP_MODEL_STRIDE;
        derive_rows(&m3, dst);
        for (int k = 0; k < 11; k++) dst[k] = models[i].transitions[k];
    }
    return append_rows(c, SM4, rows, n, nullptr, ids);
}

int cpecan_hip_models_clear(cpecan_ctx *c) {
    if (!c) return fail(CPECAN_EINVAL, "ctx is NULL");
    (void) hipSetDevice(c->device);
    (void) ctx_fence(c); /* the tables go back to the allocator's cache: no reader may be left */
    c->modelEpoch++; /* batches created before this call hold ids into tables that are gone: batch_run refuses them */
    for (ModelTable &t : c->tables) t.drop();
    hdp_tables_release(c);
    return CPECAN_OK;
}
