/*
 * cpecan_general.h -- banded forward / backward / posterior DP for bands of ANY width: the driver of the six general
 * kernels, one per state machine (cpecan_kernel_general{,4,5,v,h,e}.hip).
 *
 * One 256-thread workgroup per work item (= one getPosteriorProbsWithBanding call,
 * impl/pairwiseAligner.c:870-1006).  Threads stride over the cells of the current anti-diagonal;
 * forward diagonals are stored in HBM ([cell][state], the reference's DpDiagonal layout :567), the
 * three live backward diagonals rotate through a small HBM workspace (L2-resident).  These are the
 * correctness-first kernels and the fall-back for every batch the wave and systolic families cannot
 * take (bands wider than a wave, un-banded alignments, cell dumps, the 4-state machine).
 *
 * Differences from the reference's control flow, none of which changes a result bit:
 *   - backward is a gather (the reference scatters, :378-389); per target cell the contributions
 *     are added in the reference's order: from (d+2, xmy) [middle block], then from (d+1, xmy-1)
 *     [its upper block], then from (d+1, xmy+1) [its lower block];
 *   - a neighbour outside the band contributes -inf instead of being skipped (logAdd(a,-inf)==a);
 *   - totalProbability's sequential fold visits only the terms that change the running value
 *     (cp_wave_seq_fold).
 *
 * A machine M derives from GeneralCells<S> and supplies:
 *   start_vector(raggedL, e[S]) / end_vector(raggedEnd, e[S])   the start and end state vectors;
 *   forward_cell(d, xmy, o[S]) / backward_cell(d, dTop, xmy, o[S]) its recurrences;
 *   match_into(middle, x, y)   the match state's mass reaching cell (x, y) from the forward cell (x-1, y-1);
 *   kMultiMatch                whether states matchState..5 are all match states (the echelon machine), and then
 *   step_into(middle, x, y, o[S])  every state's mass reaching cell (x, y) from (x-1, y-1) in place of match_into,
 *                              and the decode emits s pairs per state s (diagonalCalculationMultiPosteriorMatchProbs);
 *   kDump                      whether it writes its backward cells to dbgB under P.debug;
 *   kExpect                    whether it has a Baum-Welch E-step, and then
 *   expect_diagonal(...)       what the E-step does with one posterior diagonal, and
 *   expect_fold(a, it)         the fold of its sums into `expect` at the end.
 * It may shadow lds_diagonal(d) to keep a copy of the forward diagonals for its own forward sweep.
 */
#ifndef CPECAN_GENERAL_H_
#define CPECAN_GENERAL_H_

#include "cpecan_device.h"

/* the cells of one work item: forward diagonals in HBM, the backward diagonals in the (d % 3) workspace */
template <int S_>
struct GeneralCells {
    static constexpr int S = S_;
    static constexpr bool kExpect = false; /* has a Baum-Welch E-step */
    static constexpr bool kDump = false;   /* dumps its backward cells into dbgB under P.debug */
    static constexpr bool kMultiMatch = false; /* states 1..5 are match states of s k-mers each (echelon) */
    const int *L, *R;
    const long long *pre; /* cell prefix per diagonal */
    double *F;            /* forward cells of this item */
    double *Bws;          /* 3 x maxWidth x S backward workspace */
    int maxWidth;

    __device__ GeneralCells(const DevGeneralArgs &a, const DevItem &it)
        : L(a.bandL + it.diagBase), R(a.bandR + it.diagBase), pre(a.cellPrefix + it.diagBase), F(a.F + it.cellBase * S),
          Bws(a.B + it.bwsBase), maxWidth(it.maxWidth) {}

    __device__ __forceinline__ const double *fcell(long long d, int xmy) const {
        if (d < 0) return nullptr;
        const int l = L[d], r = R[d];
        if (xmy < l || xmy > r) return nullptr;
        return F + (pre[d] + ((xmy - l) >> 1)) * S;
    }
    __device__ __forceinline__ double *bslot(long long d) const { return Bws + (d % 3) * (long long) maxWidth * S; }
    __device__ __forceinline__ const double *bcell(long long d, long long dTop, int xmy) const {
        if (d > dTop) return nullptr;
        const int l = L[d], r = R[d];
        if (xmy < l || xmy > r) return nullptr;
        return bslot(d) + ((xmy - l) >> 1) * S;
    }
    /* a second copy of forward diagonal d that the machine's forward sweep reads (none by default) */
    __device__ __forceinline__ double *lds_diagonal(long long) const { return nullptr; }
};

/* diagonalCalculationMultiPosteriorMatchProbs (impl/pairwiseAligner.c:797-839), by wave 0: per cell x-y ascending,
 * every state s = 1..5 whose posterior reaches the threshold emits s pairs (x+n-1, y-1), n = 0..s-1, with the same
 * posterior; a lane's pairs go to the slots after those of the lanes before it (a wave prefix sum of the counts) */
template <int S>
__device__ __forceinline__ void general_multi_decode(const DevGeneralArgs &a, const DevParams &P, const DevItem &it,
                                                     long long d2, int l2, int w2, const double *fdd, const double *bdd,
                                                     double total, long long &myPairs) {
    const int lane = threadIdx.x & 63;
    for (int base = 0; base < w2; base += 64) {
        const int cc = base + lane;
        double e[6];
        int cnt = 0;
        long long x = 0, y = 0;
#pragma unroll
        for (int s = 1; s < 6; s++) e[s] = CP_NEG_INF;
        unsigned hits = 0;
        if (cc < w2) {
            const int xmy = l2 + 2 * cc;
            x = (d2 + xmy) / 2;
            y = (d2 - xmy) / 2;
            if (x > 0 && y > 0) {
#pragma unroll
                for (int s = 1; s < 6; s++) {
                    e[s] = (fdd[cc * S + s] + bdd[cc * S + s]) - total;
                    if (e[s] >= P.logThrSlack) { /* (the exact threshold test is the readback's, with the host libm) */
                        hits |= 1u << s;
                        cnt += s;
                    }
                }
            }
        }
        int incl = cnt; /* inclusive prefix sum of the counts over the wave */
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int t = __shfl_up(incl, off);
            if (lane >= off) incl += t;
        }
        const int all = __shfl(incl, 63);
        long long idx = myPairs + (incl - cnt);
        for (int s = 1; s < 6; s++) {
            if (!((hits >> s) & 1u)) continue;
            double p = exp(e[s]);
            if (p > 1.0) p = 1.0;
            const long long score = (long long) floor(p * 10000000.0);
            for (int n = 0; n < s; n++, idx++) {
                if (idx < it.pairCap) {
                    long long *o = a.pairs + (it.pairBase + idx) * 3;
                    o[0] = score;
                    o[1] = x + n - 1;
                    o[2] = y - 1;
                    a.pairLogp[it.pairBase + idx] = e[s];
                }
            }
        }
        myPairs += all;
    }
}

/* one work item (blockIdx.x) through machine m */
template <class M>
__device__ __forceinline__ void general_pass(M &m, const DevGeneralArgs &a, const DevParams &P, const DevItem &it) {
    constexpr int S = M::S;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __shared__ double sTotal;

    const long long D = it.lX + it.lY;
    long long myPairs = 0, myTot = 0; /* wave-0 uniform counters */
    if (D == 0) {
        if (tid == 0) { a.nPairs[blockIdx.x] = 0; a.nTot[blockIdx.x] = 0; }
        return;
    }

    /* diagonal 0: the start state vector */
    if (tid == 0) {
        double e[S];
        m.start_vector(it.raggedL, e);
        double *fl = m.lds_diagonal(0);
#pragma unroll
        for (int s = 0; s < S; s++) {
            m.F[s] = e[s];
            if (fl) fl[s] = e[s];
        }
    }
    __threadfence_block();
    __syncthreads();

    long long tracedBackTo = 0;
    for (long long d = 1; d <= D; d++) {
        const int l = m.L[d], width = ((m.R[d] - l) >> 1) + 1;
        double *fd = m.F + m.pre[d] * S;
        double *fl = m.lds_diagonal(d);
        for (int cc = tid; cc < width; cc += 256) {
            double o[S];
            m.forward_cell(d, l + 2 * cc, o);
#pragma unroll
            for (int s = 0; s < S; s++) fd[cc * S + s] = o[s];
            if (fl)
#pragma unroll
                for (int s = 0; s < S; s++) fl[cc * S + s] = o[s];
        }
        __threadfence_block();
        __syncthreads();

        const bool atEnd = d == D;
        const bool tb = !P.unbanded && d >= tracedBackTo + P.minDiags && width <= P.expansion * 2 + 1;
        if (!(atEnd || tb)) continue;

        /* ---- traceback window (:921-992) ---- */
        const long long dTop = d;
        const long long tracedBackFrom = dTop - (atEnd ? 0 : P.tbDiags + 1);
        {
            double e[S];
            m.end_vector(atEnd && it.raggedR, e);
            double *b = m.bslot(dTop);
            for (int cc = tid; cc < width; cc += 256)
#pragma unroll
                for (int s = 0; s < S; s++) b[cc * S + s] = e[s];
        }
        __threadfence_block();
        __syncthreads();

        double total = CP_NEG_INF;
        long long calcs = 0;
        for (long long d2 = dTop; d2 > tracedBackTo; d2--) {
            const int l2 = m.L[d2], w2 = ((m.R[d2] - l2) >> 1) + 1;
            if (d2 < dTop) {
                double *b = m.bslot(d2);
                for (int cc = tid; cc < w2; cc += 256) {
                    double o[S];
                    m.backward_cell(d2, dTop, l2 + 2 * cc, o);
#pragma unroll
                    for (int s = 0; s < S; s++) b[cc * S + s] = o[s];
                }
                __threadfence_block();
                __syncthreads();
            }
            if (d2 > tracedBackFrom) continue;

            const double *fdd = m.F + m.pre[d2] * S;
            const double *bdd = m.bslot(d2);
            /* banded: refreshed every 10th posterior diagonal of the window (:956); un-banded:
             * taken once, at the last diagonal (:1556) */
            if (P.unbanded ? calcs++ == 0 : calcs++ % 10 == 0) {
                /* diagonalCalculationTotalProbability :736-754, by wave 0 */
                if (wave == 0) {
                    double acc = CP_NEG_INF;
                    for (int base = 0; base < w2; base += 64) {
                        const int cc = base + lane;
                        const bool valid = cc < w2;
                        double v = CP_NEG_INF;
                        if (valid) { /* cell_dotProduct :391-397 */
                            v = fdd[cc * S] + bdd[cc * S];
#pragma unroll
                            for (int s = 1; s < S; s++) v = cp_logAdd(v, fdd[cc * S + s] + bdd[cc * S + s]);
                        }
                        acc = cp_wave_seq_fold(acc, v, valid);
                    }
                    if (d2 + 1 <= dTop) {
                        /* matches that step over d2: forward[d2-1] --match--> cells of d2+1 */
                        const int l3 = m.L[d2 + 1], w3 = ((m.R[d2 + 1] - l3) >> 1) + 1;
                        const double *b3 = m.bslot(d2 + 1);
                        double acc2 = CP_NEG_INF;
                        for (int base = 0; base < w3; base += 64) {
                            const int cc = base + lane;
                            const bool valid = cc < w3;
                            double v = CP_NEG_INF;
                            if (valid) {
                                const int xmy = l3 + 2 * cc;
                                const double *mid = m.fcell(d2 - 1, xmy);
                                if constexpr (M::kMultiMatch) {
                                    double st[S];
#pragma unroll
                                    for (int s = 0; s < S; s++) st[s] = CP_NEG_INF;
                                    if (mid) m.step_into(mid, (d2 + 1 + xmy) / 2, (d2 + 1 - xmy) / 2, st);
                                    v = st[0] + b3[cc * S];
#pragma unroll
                                    for (int s = 1; s < S; s++) v = cp_logAdd(v, st[s] + b3[cc * S + s]);
                                } else {
                                    double mm = CP_NEG_INF;
                                    if (mid) mm = m.match_into(mid, (d2 + 1 + xmy) / 2, (d2 + 1 - xmy) / 2);
                                    v = mm + b3[cc * S];
#pragma unroll
                                    for (int s = 1; s < S; s++) v = cp_logAdd(v, CP_NEG_INF + b3[cc * S + s]);
                                }
                            }
                            acc2 = cp_wave_seq_fold(acc2, v, valid);
                        }
                        acc = cp_logAdd(acc, acc2);
                    }
                    if (lane == 0) {
                        sTotal = acc;
                        if (myTot < it.totCap) {
                            a.totXay[it.totBase + myTot] = d2;
                            a.totVal[it.totBase + myTot] = acc;
                        }
                    }
                    myTot++;
                }
                __syncthreads();
                total = sTotal;
                __syncthreads();
            }

            if constexpr (M::kDump) {
                if (P.debug && a.dbgB) {
                    double *o = a.dbgB + (it.cellBase + m.pre[d2]) * S;
                    for (int cc = tid; cc < w2 * S; cc += 256) o[cc] = bdd[cc];
                }
            }

            if constexpr (M::kExpect) {
                if (P.mode == 1) {
                    /* diagonalCalculation_Expectations :841-863; forward[d2-2] is already freed unless it lies in the
                     * window (:982) */
                    m.expect_diagonal(a, P, it, d2, l2, w2, bdd, total, d2 - 2 >= tracedBackTo, myPairs);
                    __syncthreads();
                    continue;
                }
            }
            if constexpr (M::kMultiMatch) {
                if (wave == 0) general_multi_decode<S>(a, P, it, d2, l2, w2, fdd, bdd, total, myPairs);
                __syncthreads();
                continue;
            }
            if (wave == 0) {
                /* diagonalCalculationPosteriorMatchProbs :756-795, ordered emission by wave 0 */
                for (int base = 0; base < w2; base += 64) {
                    const int cc = base + lane;
                    bool hit = false;
                    double e = 0.0, p = 0.0;
                    long long x = 0, y = 0;
                    if (cc < w2) {
                        const int xmy = l2 + 2 * cc;
                        x = (d2 + xmy) / 2;
                        y = (d2 - xmy) / 2;
                        if (x > 0 && y > 0) {
                            e = (fdd[cc * S] + bdd[cc * S]) - total;
                            p = exp(e);
                            hit = e >= P.logThrSlack; /* (the exact threshold test is the readback's, with the host libm) */
                        }
                    }
                    const unsigned long long mk = __ballot(hit);
                    if (hit) {
                        const long long idx = myPairs + __popcll(mk & ((1ull << lane) - 1ull));
                        if (idx < it.pairCap) {
                            if (p > 1.0) p = 1.0;
                            long long *o = a.pairs + (it.pairBase + idx) * 3;
                            o[0] = (long long) floor(p * 10000000.0);
                            o[1] = x - 1;
                            o[2] = y - 1;
                            a.pairLogp[it.pairBase + idx] = e;
                        }
                    }
                    myPairs += __popcll(mk);
                }
            }
            __syncthreads();
        }
        tracedBackTo = tracedBackFrom;
    }

    if constexpr (M::kExpect) {
        if (P.mode == 1 && a.expect) m.expect_fold(a, it);
    }
    if (tid == 0) {
        a.nPairs[blockIdx.x] = myPairs;
        a.nTot[blockIdx.x] = myTot;
    }
}

#endif
