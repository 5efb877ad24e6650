/*
 * cpecan_kernel_wave4.hip -- the 4-state signal machine (stateMachine4_cellCalculate, impl/stateMachine.c:867-897;
 * k-mers against events) with ONE WAVE per alignment and the recurrence in registers: posterior decode on banded
 * matrices for bands up to 64 * L cells (L = 1, 2 cells per lane; the reference's driver runs this machine at
 * diagonalExpansion 50, bands of about 100 cells).  Opt-in: CPECAN_FLAG_SM4_WAVE.
 *
 * The shape is that of cpecan_kernel_wave5.hip (its one-wave form; no wave here waits for another):
 *   - slots are anchored to the matrix column: slot = x mod (64 * L), lane = slot / L.  A lane keeps its slots' four
 *     forward values of d-1 and one copy each of its lower neighbour's on d-1 and d-2, so a diagonal costs ONE lane
 *     shift of four values; every neighbour is guarded by the band of its own diagonal (bandL / bandR), so a slot that
 *     changed hands is never read and band edges may step by more than one;
 *   - forward cells go to the general kernel's [cell][state] layout in HBM; the traceback window is swept back in the
 *     same launch, the backward cells of d+1 and d+2 held the same way (neighbours at slot + 1); the ordered folds of
 *     diagonalCalculationTotalProbability (impl/pairwiseAligner.c:736-754) and the ordered emission of the pairs
 *     (:756-795) go through an LDS staging row in x order.
 * What differs is the emission: a slot's k-mer row is the thirteen doubles of the strawMan table the machine reads (the
 * match Gaussians, the extra-event Gaussians, the gap-X probability), loaded when the slot takes a new column and kept
 * in registers; its event advances by one every diagonal (y = d - x) and is requested a diagonal ahead, as is the k-mer
 * index of the column it will hold then.  The sweep back reads the match half and gap-X of row x and the extra-event
 * half of row x-1: thirteen doubles again.
 * Arithmetic, its order and the outputs are those of cpecan_kernel_general4.hip (Sm4::forward_cell, ::backward_cell) and
 * of the reference; index -1 reads the "not a k-mer" row 4096 and the -inf event, as there.  Un-banded calls and wider
 * bands stay on the general kernel.
 */
#include "cpecan_device.h"

namespace {

enum { /* _StateMachine4's members in order (inc/stateMachine.h:134-152) */
    T4_MATCH_CONTINUE = 0, T4_MATCH_FROM_SHORT_GAP_X, T4_MATCH_FROM_LONG_GAP_X, T4_MATCH_FROM_SHORT_GAP_Y,
    T4_GAP_SHORT_OPEN_X, T4_GAP_SHORT_EXTEND_X, T4_GAP_SHORT_OPEN_Y, T4_GAP_SHORT_EXTEND_Y,
    T4_GAP_LONG_OPEN_X, T4_GAP_LONG_EXTEND_X, T4_GAP_LONG_SWITCH_TO_X
};
#define W4S 4
/* a row in registers: [mu sd K1 nmu nsd K2] of the match table, the same of the extra-event table, gap X */
#define W4_M 0
#define W4_Y 6
#define W4_GAPX 12
#define W4_ROW 13

/* logAdd without branches, cp_logAdd's value bit for bit (cpecan_kernel_wave5.hip: w5_ladd_t, and why it is exact) */
__device__ __forceinline__ double w4_ladd_t(double x, double y, const double *coef) {
    const bool xs = x < y;
    const double hi = xs ? y : x, lo = xs ? x : y;
    const double d = hi - lo;
    const bool near = d < 7.5;
    const int n = near ? (int) __builtin_ceil(d + d) : 15;
    const double *c = coef + 4 * n;
    const double r = (((c[0] * d + c[1]) * d + c[2]) * d + c[3]) + lo;
    return near ? r : hi;
}
__device__ __forceinline__ void w4_init_coef(double *coef) {
    const float t[16] = { -0.009350833524763f, 0.130659527668286f, 0.498799810682272f, 0.693203116424741f,
                          -0.014532321752540f, 0.139942324101744f, 0.495635523139337f, 0.692140569840976f,
                          -0.004605031767994f, 0.063427417320019f, 0.695956496475118f, 0.514272634594009f,
                          -0.000458661602210f, 0.009695946122598f, 0.930734667215156f, 0.168037164329057f };
    const int l = threadIdx.x & 63, n = l >> 2, piece = n <= 2 ? 0 : n <= 5 ? 1 : n <= 9 ? 2 : 3;
    coef[l] = (double) t[piece * 4 + (l & 3)];
}
#define cp_logAdd(a, b) w4_ladd_t((a), (b), coef) /* (everything below, where `coef` is the LDS table; the sequential
                                                       folds of cpecan_device.h keep their own) */
/* a wave runs in lockstep and its LDS operations execute in order: all that is needed is that the compiler keeps the
 * order (a fence at wavefront scope is no instruction) */
__device__ __forceinline__ void w4_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
/* the matrix column slot `sl` holds on a diagonal whose band is [xmin, xmax] (at most P columns), or -1 */
template <int P> __device__ __forceinline__ int w4_column(int sl, int xmin, int xmax) {
    int x = xmin + ((sl - xmin) % P + P) % P;
    return x <= xmax ? x : -1;
}
/* Sm4::row4's index and Sm4::event4 (cpecan_kernel_general4.hip); an index past the sequence is never a cell's: it
 * reads the sentinel too */
__device__ __forceinline__ int w4_kmer(const unsigned short *kidx, long long ix, long long lX) {
    return ix >= 0 && ix < lX ? (int) kidx[ix] : 4096;
}
__device__ __forceinline__ void w4_event(const double *ev, long long iy, long long lY, double &mean, double &noise) {
    if (iy >= 0 && iy < lY) { mean = ev[3 * iy]; noise = ev[3 * iy + 1]; }
    else { mean = CP_NEG_INF; noise = 0.0; }
}
/* emissions_signal_strawManGetKmerEventMatchProb (impl/stateMachine.c:595-629) over six doubles of a row */
__device__ __forceinline__ double w4_emit(const double *r, double mean, double noise) {
    return cp_logGauss(mean, r[0], r[1], r[2]) + cp_logGauss(noise, r[3], r[4], r[5]);
}
__device__ __forceinline__ void w4_load_match(double *r, const double *row) {
    r[0] = row[CP_MU]; r[1] = row[CP_SD]; r[2] = row[CP_K1];
    r[3] = row[CP_NMU]; r[4] = row[CP_NSD]; r[5] = row[CP_K2];
}
__device__ __forceinline__ void w4_load_extra(double *r, const double *row) {
    r[0] = row[CP_YMU]; r[1] = row[CP_YSD]; r[2] = row[CP_YK1];
    r[3] = row[CP_YNMU]; r[4] = row[CP_YNSD]; r[5] = row[CP_YK2];
}
__device__ __forceinline__ double w4_match_from(const double *middle, double eP, const double *t, const double *coef) {
    double m = CP_NEG_INF;
    m = cp_logAdd(m, middle[0] + (eP + t[T4_MATCH_CONTINUE]));
    m = cp_logAdd(m, middle[1] + (eP + t[T4_MATCH_FROM_SHORT_GAP_X]));
    m = cp_logAdd(m, middle[2] + (eP + t[T4_MATCH_FROM_SHORT_GAP_Y]));
    m = cp_logAdd(m, middle[3] + (eP + t[T4_MATCH_FROM_LONG_GAP_X]));
    return m;
}

template <int L> __device__ __forceinline__ void wave4_body(
    const DevItem &it, const DevParams &P, const int *__restrict__ bandL, const int *__restrict__ bandR,
    const long long *__restrict__ pre, const unsigned short *__restrict__ kidx, const double *__restrict__ ev,
    const double *__restrict__ model, double *F, long long *pairs, double *pairLogp, long long *totXay, double *totVal,
    long long &myPairs, long long &myTot, double *stage /* LDS, 64 * L doubles */, const double *coef /* LDS */) {
    constexpr int PP = 64 * L;
    const int lane = threadIdx.x & 63;
    const double *t = model, *rows = model + CP_MODEL_HEADER;
    const long long D = it.lX + it.lY, lX = it.lX, lY = it.lY;

    /* forward state per slot: own cell on d-1, the lower neighbour's cells on d-1 and d-2 */
    double U[L][W4S], N2[L][W4S];
#pragma unroll
    for (int j = 0; j < L; j++)
#pragma unroll
        for (int s = 0; s < W4S; s++) U[j][s] = N2[j][s] = CP_NEG_INF;
    /* diagonal 0: stateMachine5_startStateProb / stateMachine4_raggedStartStateProb (:743, :791); column 0 = slot 0 */
    if (lane == 0) {
        U[0][0] = it.raggedL ? CP_NEG_INF : 0.0;
        U[0][1] = CP_NEG_INF;
        U[0][2] = it.raggedL ? 0.0 : CP_NEG_INF;
        U[0][3] = it.raggedL ? 0.0 : CP_NEG_INF;
#pragma unroll
        for (int s = 0; s < W4S; s++) F[s] = U[0][s];
    }

    long long tracedBackTo = 0;
    int xmin1 = 0, xmax1 = 0;   /* band of d-1 (diagonal 0: the single column 0) */
    int xmin2 = 0, xmax2 = -1;  /* band of d-2 (none yet) */
    /* nothing the sweep loads may sit on its critical path: the band row and the cell prefix of the next diagonal, and
     * every slot's next event and the k-mer index of its next column, are fetched a diagonal ahead; the row itself
     * only changes when the slot changes hands */
    int nLo = bandL[1], nHi = bandR[1];
    long long nPre = pre[1];
    int colX[L], nextK[L];
    double row[L][W4_ROW], nextMean[L], nextNoise[L];
#pragma unroll
    for (int j = 0; j < L; j++) {
        colX[j] = -2;
#pragma unroll
        for (int k = 0; k < W4_ROW; k++) row[j][k] = 0.0;
        const int x = w4_column<PP>(lane * L + j, (int) ((1 + nLo) / 2), (int) ((1 + nHi) / 2));
        w4_event(ev, x >= 0 ? (1 - (long long) x) - 1 : -1, lY, nextMean[j], nextNoise[j]);
        nextK[j] = x >= 0 ? w4_kmer(kidx, (long long) x - 1, lX) : 4096;
    }
    for (long long d = 1; d <= D; d++) {
        const int lo = nLo, hi = nHi;
        const long long preD = nPre;
        const int xmin = (int) ((d + lo) / 2), xmax = (int) ((d + hi) / 2), width = xmax - xmin + 1;
        if (d < D) {
            nLo = bandL[d + 1];
            nHi = bandR[d + 1];
            nPre = pre[d + 1];
        }
        double mean[L], noise[L];
        int km[L];
#pragma unroll
        for (int j = 0; j < L; j++) {
            mean[j] = nextMean[j];
            noise[j] = nextNoise[j];
            km[j] = nextK[j];
        }
        if (d < D) {
            const int nxmin = (int) ((d + 1 + nLo) / 2), nxmax = (int) ((d + 1 + nHi) / 2);
#pragma unroll
            for (int j = 0; j < L; j++) {
                const int x = w4_column<PP>(lane * L + j, nxmin, nxmax);
                w4_event(ev, x >= 0 ? (d + 1 - (long long) x) - 1 : -1, lY, nextMean[j], nextNoise[j]);
                nextK[j] = x >= 0 ? w4_kmer(kidx, (long long) x - 1, lX) : 4096;
            }
        }
        /* the lower neighbour's cells of d-1: slot - 1 is the previous layer of the lane, or the last layer of the
         * lane below */
        double N1[L][W4S];
#pragma unroll
        for (int s = 0; s < W4S; s++) {
            const double below = __shfl(U[L - 1][s], (lane + 63) & 63);
#pragma unroll
            for (int j = L - 1; j >= 1; j--) N1[j][s] = U[j - 1][s];
            N1[0][s] = below;
        }
        double *fd = F + preD * W4S;
        double Uo[L][W4S];
#pragma unroll
        for (int j = 0; j < L; j++) {
            const int x = w4_column<PP>(lane * L + j, xmin, xmax);
            double o[W4S];
#pragma unroll
            for (int s = 0; s < W4S; s++) o[s] = CP_NEG_INF;
            if (x >= 0) {
                if (x != colX[j]) { /* row4(x - 1) */
                    colX[j] = x;
                    const double *r = rows + (long long) km[j] * CP_ROW;
                    w4_load_match(row[j] + W4_M, r);
                    w4_load_extra(row[j] + W4_Y, r);
                    row[j][W4_GAPX] = r[CP_GAPX];
                }
                const bool lower = x - 1 >= xmin1 && x - 1 <= xmax1;
                const bool middle = d >= 2 && x - 1 >= xmin2 && x - 1 <= xmax2;
                const bool upper = x >= xmin1 && x <= xmax1;
                if (lower) {
                    const double eP = row[j][W4_GAPX];
                    o[1] = cp_logAdd(o[1], N1[j][0] + (eP + t[T4_GAP_SHORT_OPEN_X]));
                    o[1] = cp_logAdd(o[1], N1[j][1] + (eP + t[T4_GAP_SHORT_EXTEND_X]));
                    o[3] = cp_logAdd(o[3], N1[j][0] + (eP + t[T4_GAP_LONG_OPEN_X]));
                    o[3] = cp_logAdd(o[3], N1[j][3] + (eP + t[T4_GAP_LONG_EXTEND_X]));
                    o[3] = cp_logAdd(o[3], N1[j][2] + (eP + t[T4_GAP_LONG_SWITCH_TO_X]));
                }
                if (middle) o[0] = w4_match_from(N2[j], w4_emit(row[j] + W4_M, mean[j], noise[j]), t, coef);
                if (upper) {
                    const double eP = w4_emit(row[j] + W4_Y, mean[j], noise[j]);
                    o[2] = cp_logAdd(o[2], U[j][0] + (eP + t[T4_GAP_SHORT_OPEN_Y]));
                    o[2] = cp_logAdd(o[2], U[j][2] + (eP + t[T4_GAP_SHORT_EXTEND_Y]));
                }
                double *dst = fd + (long long) (x - xmin) * W4S;
#pragma unroll
                for (int s = 0; s < W4S; s++) dst[s] = o[s];
            }
#pragma unroll
            for (int s = 0; s < W4S; s++) {
                N2[j][s] = N1[j][s]; /* (the lower neighbour's d-1 is its d-2 a diagonal later) */
                Uo[j][s] = o[s];
            }
        }
#pragma unroll
        for (int j = 0; j < L; j++)
#pragma unroll
            for (int s = 0; s < W4S; s++) U[j][s] = Uo[j][s];
        xmin2 = xmin1; xmax2 = xmax1;
        xmin1 = xmin; xmax1 = xmax;

        const bool atEnd = d == D;
        const bool tb = d >= tracedBackTo + P.minDiags && width <= P.expansion * 2 + 1;
        if (!(atEnd || tb)) continue;

        /* ---- traceback window (:921-992) ---- */
        const long long dTop = d;
        const long long tracedBackFrom = dTop - (atEnd ? 0 : P.tbDiags + 1);
        __threadfence_block(); /* the window's forward cells are read back from HBM below */
        double e[W4S]; /* stateMachine4_endStateProb / _raggedEndStateProb (:796-829) */
        if (atEnd && it.raggedR) {
            e[0] = e[1] = e[2] = t[T4_GAP_LONG_OPEN_X];
            e[3] = t[T4_GAP_LONG_EXTEND_X];
        } else {
            e[0] = t[T4_MATCH_CONTINUE];
            e[1] = t[T4_MATCH_FROM_SHORT_GAP_X];
            e[2] = t[T4_MATCH_FROM_SHORT_GAP_Y];
            e[3] = t[T4_MATCH_FROM_LONG_GAP_X];
        }
        /* backward state per slot: own cell on d2+1 (Bo), the upper-slot neighbour's cells on d2+1 and d2+2 */
        double Bo[L][W4S], Bn2[L][W4S];
#pragma unroll
        for (int j = 0; j < L; j++)
#pragma unroll
            for (int s = 0; s < W4S; s++) Bo[j][s] = Bn2[j][s] = CP_NEG_INF;
        int bxmin1 = 0, bxmax1 = -1, bxmin2 = 0, bxmax2 = -1; /* bands of d2+1 and d2+2 (none above dTop) */
        double total = CP_NEG_INF;
        long long calcs = 0;
        /* as on the way up, what the sweep loads is fetched a diagonal ahead: the band row and cell prefix, every
         * slot's event, the k-mer indices of its column and the match-state forward value of its cell (the other
         * three states are only read on the one diagonal in ten that refreshes the total).  Of a cell (x, y) the
         * sweep back reads event y, the match half and gap X of row4(x) and the extra-event half of row4(x - 1). */
        int qLo = lo, qHi = hi;
        long long qPre = preD;
        int colB[L], nextKm[L], nextKy[L];
        double rowM[L][7], rowY[L][6], nextMeanB[L], nextNoiseB[L], nextF0[L];
#pragma unroll
        for (int j = 0; j < L; j++) {
            colB[j] = -2;
#pragma unroll
            for (int k = 0; k < 7; k++) rowM[j][k] = 0.0;
#pragma unroll
            for (int k = 0; k < 6; k++) rowY[j][k] = 0.0;
            const int x = w4_column<PP>(lane * L + j, xmin, xmax);
            w4_event(ev, x >= 0 ? dTop - (long long) x : -1, lY, nextMeanB[j], nextNoiseB[j]);
            nextKm[j] = x >= 0 ? w4_kmer(kidx, (long long) x, lX) : 4096;
            nextKy[j] = x >= 0 ? w4_kmer(kidx, (long long) x - 1, lX) : 4096;
            nextF0[j] = U[j][0]; /* the forward cells of dTop are still in registers */
        }
        for (long long d2 = dTop; d2 > tracedBackTo; d2--) {
            const int l2 = qLo, h2 = qHi;
            const long long pre2 = qPre;
            const int cxmin = (int) ((d2 + l2) / 2), cxmax = (int) ((d2 + h2) / 2), w2 = cxmax - cxmin + 1;
            double meanB[L], noiseB[L], f0[L];
            int kM[L], kY[L];
#pragma unroll
            for (int j = 0; j < L; j++) {
                meanB[j] = nextMeanB[j];
                noiseB[j] = nextNoiseB[j];
                f0[j] = nextF0[j];
                kM[j] = nextKm[j];
                kY[j] = nextKy[j];
            }
            if (d2 - 1 > tracedBackTo) {
                qLo = bandL[d2 - 1];
                qHi = bandR[d2 - 1];
                qPre = pre[d2 - 1];
                const int nxmin = (int) ((d2 - 1 + qLo) / 2), nxmax = (int) ((d2 - 1 + qHi) / 2);
#pragma unroll
                for (int j = 0; j < L; j++) {
                    const int x = w4_column<PP>(lane * L + j, nxmin, nxmax);
                    w4_event(ev, x >= 0 ? d2 - 1 - (long long) x : -1, lY, nextMeanB[j], nextNoiseB[j]);
                    nextKm[j] = x >= 0 ? w4_kmer(kidx, (long long) x, lX) : 4096;
                    nextKy[j] = x >= 0 ? w4_kmer(kidx, (long long) x - 1, lX) : 4096;
                    nextF0[j] = (x >= 0 && d2 - 1 <= tracedBackFrom) ? F[(qPre + (x - nxmin)) * W4S] : 0.0;
                }
            }
            /* the upper-slot neighbour's cells of d2+1: slot + 1 is the next layer of the lane, or the first layer of
             * the lane above */
            double cur[L][W4S], Bn1[L][W4S];
#pragma unroll
            for (int s = 0; s < W4S; s++) {
                const double above = __shfl(Bo[0][s], (lane + 1) & 63);
#pragma unroll
                for (int j = 0; j + 1 < L; j++) Bn1[j][s] = Bo[j + 1][s];
                Bn1[L - 1][s] = above;
            }
#pragma unroll
            for (int j = 0; j < L; j++) {
                const int x = w4_column<PP>(lane * L + j, cxmin, cxmax);
                if (x >= 0 && x != colB[j]) {
                    colB[j] = x;
                    const double *rm = rows + (long long) kM[j] * CP_ROW, *ry = rows + (long long) kY[j] * CP_ROW;
                    w4_load_match(rowM[j], rm);
                    rowM[j][6] = rm[CP_GAPX];
                    w4_load_extra(rowY[j], ry);
                }
#pragma unroll
                for (int s = 0; s < W4S; s++) cur[j][s] = d2 == dTop ? e[s] : CP_NEG_INF;
                if (x >= 0 && d2 < dTop) {
                    /* (ii) cell (x+1, y+1) on d2+2 reaches this cell through its middle block */
                    if (d2 + 2 <= dTop && x + 1 >= bxmin2 && x + 1 <= bxmax2) {
                        const double eP = w4_emit(rowM[j], meanB[j], noiseB[j]);
                        const double s20 = Bn2[j][0];
                        cur[j][0] = cp_logAdd(cur[j][0], s20 + (eP + t[T4_MATCH_CONTINUE]));
                        cur[j][1] = cp_logAdd(cur[j][1], s20 + (eP + t[T4_MATCH_FROM_SHORT_GAP_X]));
                        cur[j][2] = cp_logAdd(cur[j][2], s20 + (eP + t[T4_MATCH_FROM_SHORT_GAP_Y]));
                        cur[j][3] = cp_logAdd(cur[j][3], s20 + (eP + t[T4_MATCH_FROM_LONG_GAP_X]));
                    }
                    /* (iii) cell (x, y+1) on d2+1 reaches it through its upper block */
                    if (x >= bxmin1 && x <= bxmax1) {
                        const double eP = w4_emit(rowY[j], meanB[j], noiseB[j]);
                        cur[j][0] = cp_logAdd(cur[j][0], Bo[j][2] + (eP + t[T4_GAP_SHORT_OPEN_Y]));
                        cur[j][2] = cp_logAdd(cur[j][2], Bo[j][2] + (eP + t[T4_GAP_SHORT_EXTEND_Y]));
                    }
                    /* (iv) cell (x+1, y) on d2+1 reaches it through its lower block */
                    if (x + 1 >= bxmin1 && x + 1 <= bxmax1) {
                        const double eP = rowM[j][6];
                        cur[j][0] = cp_logAdd(cur[j][0], Bn1[j][1] + (eP + t[T4_GAP_SHORT_OPEN_X]));
                        cur[j][1] = cp_logAdd(cur[j][1], Bn1[j][1] + (eP + t[T4_GAP_SHORT_EXTEND_X]));
                        cur[j][0] = cp_logAdd(cur[j][0], Bn1[j][3] + (eP + t[T4_GAP_LONG_OPEN_X]));
                        cur[j][3] = cp_logAdd(cur[j][3], Bn1[j][3] + (eP + t[T4_GAP_LONG_EXTEND_X]));
                        cur[j][2] = cp_logAdd(cur[j][2], Bn1[j][3] + (eP + t[T4_GAP_LONG_SWITCH_TO_X]));
                    }
                }
            }

            if (d2 <= tracedBackFrom) {
                const double *fdd = F + pre2 * W4S;
                if (calcs++ % 10 == 0) {
                    /* diagonalCalculationTotalProbability :736-754: the cells' dot products folded in x order */
                    w4_wave_sync();
#pragma unroll
                    for (int j = 0; j < L; j++) {
                        const int x = w4_column<PP>(lane * L + j, cxmin, cxmax);
                        if (x >= 0) {
                            const double *f = fdd + (long long) (x - cxmin) * W4S;
                            double v = f[0] + cur[j][0]; /* cell_dotProduct :391-397 */
#pragma unroll
                            for (int s = 1; s < W4S; s++) v = cp_logAdd(v, f[s] + cur[j][s]);
                            stage[x - cxmin] = v;
                        }
                    }
                    w4_wave_sync();
                    double acc = CP_NEG_INF;
                    for (int base = 0; base < w2; base += 64) {
                        const int cc = base + lane;
                        acc = cp_wave_seq_fold(acc, cc < w2 ? stage[cc] : CP_NEG_INF, cc < w2);
                    }
                    if (d2 + 1 <= dTop) {
                        /* matches that step over d2: forward[d2-1] --match--> cells of d2+1 (whose backward values
                         * are the own-slot registers Bo).  The band of d2-1, the match row of x-1 and event y-1 are
                         * loaded here as general_pass / match_into load them, although the look-ahead holds the
                         * band of d2-1 whenever d2-1 lies in the window: this runs on one decoded diagonal in ten,
                         * also at the window's last one where the look-ahead has nothing, and the slots here are
                         * those of d2+1, whose columns are not the ones the row and event registers hold */
                        const int w3 = bxmax1 - bxmin1 + 1;
                        w4_wave_sync();
#pragma unroll
                        for (int j = 0; j < L; j++) {
                            const int x = w4_column<PP>(lane * L + j, bxmin1, bxmax1);
                            if (x >= 0) {
                                const long long y = d2 + 1 - x;
                                double m = CP_NEG_INF;
                                const long long dm = d2 - 1;
                                if (dm >= 0) {
                                    const int ml = bandL[dm], mh = bandR[dm];
                                    const int mxmin = (int) ((dm + ml) / 2), mxmax = (int) ((dm + mh) / 2);
                                    if (x - 1 >= mxmin && x - 1 <= mxmax) {
                                        const double *mid = F + (pre[dm] + (x - 1 - mxmin)) * W4S;
                                        double rm[6], mn, ns;
                                        w4_load_match(rm, rows + (long long) w4_kmer(kidx, (long long) x - 1, lX) * CP_ROW);
                                        w4_event(ev, y - 1, lY, mn, ns);
                                        m = w4_match_from(mid, w4_emit(rm, mn, ns), t, coef);
                                    }
                                }
                                double v = m + Bo[j][0];
#pragma unroll
                                for (int s = 1; s < W4S; s++) v = cp_logAdd(v, CP_NEG_INF + Bo[j][s]);
                                stage[x - bxmin1] = v;
                            }
                        }
                        w4_wave_sync();
                        double acc2 = CP_NEG_INF;
                        for (int base = 0; base < w3; base += 64) {
                            const int cc = base + lane;
                            acc2 = cp_wave_seq_fold(acc2, cc < w3 ? stage[cc] : CP_NEG_INF, cc < w3);
                        }
                        acc = cp_logAdd(acc, acc2);
                    }
                    if (lane == 0 && myTot < it.totCap) {
                        totXay[it.totBase + myTot] = d2;
                        totVal[it.totBase + myTot] = acc;
                    }
                    myTot++;
                    total = acc;
                }

                /* diagonalCalculationPosteriorMatchProbs :756-795, emitted in x order */
                w4_wave_sync();
#pragma unroll
                for (int j = 0; j < L; j++) {
                    const int x = w4_column<PP>(lane * L + j, cxmin, cxmax);
                    if (x >= 0) stage[x - cxmin] = f0[j] + cur[j][0];
                }
                w4_wave_sync();
                for (int base = 0; base < w2; base += 64) {
                    const int cc = base + lane;
                    bool hit = false;
                    double ee = 0.0, p = 0.0;
                    long long x = 0, y = 0;
                    if (cc < w2) {
                        x = cxmin + cc;
                        y = d2 - x;
                        if (x > 0 && y > 0) {
                            ee = stage[cc] - total;
                            p = exp(ee);
                            hit = ee >= P.logThrSlack; /* (the exact threshold test is the readback's, with the host libm) */
                        }
                    }
                    const unsigned long long m = __ballot(hit);
                    if (hit) {
                        const long long idx = myPairs + __popcll(m & ((1ull << lane) - 1ull));
                        if (idx < it.pairCap) {
                            if (p > 1.0) p = 1.0;
                            long long *o = pairs + (it.pairBase + idx) * 3;
                            o[0] = (long long) floor(p * 10000000.0);
                            o[1] = x - 1;
                            o[2] = y - 1;
                            pairLogp[it.pairBase + idx] = ee;
                        }
                    }
                    myPairs += __popcll(m);
                }
            }

            /* one diagonal down: the upper-slot neighbour's d2+1 becomes its d2+2, this diagonal becomes d2+1 */
#pragma unroll
            for (int s = 0; s < W4S; s++)
#pragma unroll
                for (int j = 0; j < L; j++) {
                    Bn2[j][s] = Bn1[j][s];
                    Bo[j][s] = cur[j][s];
                }
            bxmin2 = bxmin1; bxmax2 = bxmax1;
            bxmin1 = cxmin; bxmax1 = cxmax;
        }
        tracedBackTo = tracedBackFrom;
        /* the forward sweep loads its rows and what it had fetched ahead again: they do not hold registers while a
         * window is swept back */
        const int nxmin = (int) ((d + 1 + nLo) / 2), nxmax = (int) ((d + 1 + nHi) / 2);
#pragma unroll
        for (int j = 0; j < L; j++) {
            colX[j] = -2;
#pragma unroll
            for (int k = 0; k < W4_ROW; k++) row[j][k] = 0.0;
            const int x = d < D ? w4_column<PP>(lane * L + j, nxmin, nxmax) : -1;
            w4_event(ev, x >= 0 ? (d + 1 - (long long) x) - 1 : -1, lY, nextMean[j], nextNoise[j]);
            nextK[j] = x >= 0 ? w4_kmer(kidx, (long long) x - 1, lX) : 4096;
        }
    }
}

} // namespace

/* two waves per SIMD at least: 256 registers */
#define W4_KERNEL(L, NAME)                                                                                        \
    extern "C" __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) void NAME(DevGeneralArgs a, \
                                                                                                   DevParams P) { \
        __shared__ double stage[64 * L];                                                                          \
        __shared__ double coefTable[64];                                                                          \
        w4_init_coef(coefTable);                                                                                  \
        w4_wave_sync();                                                                                           \
        const DevItem it = a.items[blockIdx.x];                                                                   \
        long long myPairs = 0, myTot = 0;                                                                         \
        if (it.lX + it.lY > 0)                                                                                    \
            wave4_body<L>(it, P, a.bandL + it.diagBase, a.bandR + it.diagBase, a.cellPrefix + it.diagBase,        \
                          (const unsigned short *) a.x + it.xOff, (const double *) a.y + 3 * it.yOff,             \
                          (const double *) a.models + (long long) it.model * CP_MODEL_STRIDE,                     \
                          a.F + it.cellBase * W4S, a.pairs, a.pairLogp, a.totXay, a.totVal, myPairs, myTot, stage, \
                          coefTable);                                                                             \
        if (threadIdx.x == 0) {                                                                                   \
            a.nPairs[blockIdx.x] = myPairs;                                                                       \
            a.nTot[blockIdx.x] = myTot;                                                                           \
        }                                                                                                         \
    }
W4_KERNEL(1, cpecan_k_wave4_l1)
W4_KERNEL(2, cpecan_k_wave4_l2)
