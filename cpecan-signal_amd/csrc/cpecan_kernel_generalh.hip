/*
 * cpecan_kernel_generalh.hip -- banded forward / backward / posterior DP for the reference's 3-state
 * HDP signal machine (stateMachine3HDP_cellCalculate, impl/stateMachine.c:1336-1366; SURVEY R13,
 * BASELINE configs[4]): the 3-state transitions of the strawMan machine, X-gap emission log(0.1),
 * match and Y-gap emission = the posterior-predictive density of the k-mer's Dirichlet process at the
 * event mean (get_nanopore_kmer_density impl/nanopore_hdp.c:390 -> dir_proc_density impl/hdp.c:2577
 * -> grid_spline_interp impl/hdp_math_utils.c:471) -- a linear density used where a log-probability
 * is expected, exactly as the reference does (quirk Q6).  X elements are read as sequence_getKmer3
 * does (impl/pairwiseAligner.c:327-331).
 *
 * On the general driver (cpecan_general.h): any band width, posterior decode and Baum-Welch
 * expectations with event assignments.  The spline tables (values and slopes on the sampling grid, one row per OBSERVED Dirichlet process) stay in
 * HBM; a cell gathers four doubles from the row of its k-mer's nearest observed ancestor, which the
 * host resolved per k-mer id when the model was uploaded.
 */
#include "cpecan_general.h"

namespace {

#define GAPX_EP (-2.3025850929940455) /* log(0.1), stateMachine.c:1347 */

__device__ __forceinline__ double match_fromh(const double *middle, double eP, const double *t) {
    double m = CP_NEG_INF;
    m = cp_logAdd(m, middle[0] + (eP + t[T_MATCH_CONTINUE]));
    m = cp_logAdd(m, middle[1] + (eP + t[T_MATCH_FROM_GAP_X]));
    m = cp_logAdd(m, middle[2] + (eP + t[T_MATCH_FROM_GAP_Y]));
    return m;
}

struct Hdp : GeneralCells<3> {
    static constexpr bool kExpect = true;
    const int *kid;     /* k-mer id (over the model's alphabet) per X character position; -1: bad character */
    const double *ev;   /* events, 3 doubles each */
    DevHdpModel model;
    double expAcc[10];  /* per-thread partial expectations: 9 transitions + likelihood */
    double *sExp;       /* [16] in LDS: the block reduction of expAcc */

    __device__ Hdp(const DevGeneralArgs &a, const DevItem &it, double *sExp_) : GeneralCells<3>(a, it), sExp(sExp_) {
        kid = (const int *) a.x + it.xOff;
        ev = (const double *) a.y + 3 * it.yOff;
        model = ((const DevHdpModel *) a.models)[it.model];
        for (int i = 0; i < 10; i++) expAcc[i] = 0.0;
    }

    /* grid_spline_interp (evenly spaced grid), then the clamp of dir_proc_density */
    __device__ __forceinline__ double density(long long ix, long long iy) const {
        const int id = kid[ix >= 0 ? ix : 0]; /* sequence_getKmer3: index < 0 reads the first k-mer */
        const double q = iy >= 0 ? ev[3 * iy] : CP_NEG_INF; /* NULLEVENT mean */
        if (id < 0) return q - q; /* NaN: the reference exits on a character outside the alphabet */
        const long long row = model.kmerRow[id];
        const double *x = model.grid, *y = model.y + row * model.gridLength, *s = model.slope + row * model.gridLength;
        const int n = model.gridLength - 1;
        double r;
        if (q <= x[0]) r = y[0] - s[0] * (x[0] - q);
        else if (q >= x[n]) r = y[n] + s[n] * (q - x[n]);
        else {
            const double dx = x[1] - x[0];
            const long long il = (long long) ((q - x[0]) / dx), ir = il + 1;
            const double dy = y[ir] - y[il];
            const double a = s[il] * dx - dy;
            const double b = dy - s[ir] * dx;
            const double tl = (q - x[il]) / dx;
            const double tr = 1.0 - tl;
            r = tr * y[il] + tl * y[ir] + tl * tr * (a * tr + b * tl);
        }
        return r > 0.0 ? r : 0.0;
    }
    __device__ __forceinline__ double match_into(const double *middle, long long x, long long y) const {
        return match_fromh(middle, density(x - 1, y - 1), model.t);
    }

    /* stateMachine3_startStateProb / raggedStartStateProb (:1168-1177), shared with sm3 */
    __device__ __forceinline__ void start_vector(bool ragged, double e[3]) const {
        e[0] = ragged ? CP_NEG_INF : 0.0;
        e[1] = ragged ? 0.0 : CP_NEG_INF;
        e[2] = ragged ? 0.0 : CP_NEG_INF;
    }
    /* stateMachine3_endStateProb / raggedEndStateProb (:1179-1207) */
    __device__ __forceinline__ void end_vector(bool ragged, double e[3]) const {
        const double *t = model.t;
        if (ragged) {
            e[0] = (t[T_GAP_OPEN_X] + t[T_GAP_OPEN_Y]) / 2.0;
            e[1] = t[T_GAP_EXTEND_X];
            e[2] = t[T_GAP_EXTEND_Y];
        } else {
            e[0] = t[T_MATCH_CONTINUE];
            e[1] = t[T_MATCH_FROM_GAP_X];
            e[2] = t[T_MATCH_FROM_GAP_Y];
        }
    }

    __device__ __forceinline__ void forward_cell(long long d, int xmy, double o[3]) const {
        const long long x = (d + xmy) / 2, y = (d - xmy) / 2;
        const double *t = model.t;
        o[0] = o[1] = o[2] = CP_NEG_INF;
        const double *lower = fcell(d - 1, xmy - 1);
        const double *middle = fcell(d - 2, xmy);
        const double *upper = fcell(d - 1, xmy + 1);
        if (lower) {
            o[1] = cp_logAdd(o[1], lower[0] + (GAPX_EP + t[T_GAP_OPEN_X]));
            o[1] = cp_logAdd(o[1], lower[1] + (GAPX_EP + t[T_GAP_EXTEND_X]));
            o[1] = cp_logAdd(o[1], lower[2] + (GAPX_EP + t[T_GAP_SWITCH_TO_X]));
        }
        if (middle) o[0] = match_fromh(middle, density(x - 1, y - 1), t);
        if (upper) {
            const double eP = density(x - 1, y - 1);
            o[2] = cp_logAdd(o[2], upper[0] + (eP + t[T_GAP_OPEN_Y]));
            o[2] = cp_logAdd(o[2], upper[2] + (eP + t[T_GAP_EXTEND_Y]));
        }
    }

    /* gather form of cell_calculateBackward, the reference's scatter order kept per target state */
    __device__ __forceinline__ void backward_cell(long long d, long long dTop, int xmy, double o[3]) const {
        const long long x = (d + xmy) / 2, y = (d - xmy) / 2;
        const double *t = model.t;
        o[0] = o[1] = o[2] = CP_NEG_INF;
        const double *s2 = bcell(d + 2, dTop, xmy);
        if (s2) {
            const double eP = density(x, y);
            o[0] = cp_logAdd(o[0], s2[0] + (eP + t[T_MATCH_CONTINUE]));
            o[1] = cp_logAdd(o[1], s2[0] + (eP + t[T_MATCH_FROM_GAP_X]));
            o[2] = cp_logAdd(o[2], s2[0] + (eP + t[T_MATCH_FROM_GAP_Y]));
        }
        const double *su = bcell(d + 1, dTop, xmy - 1);
        if (su) {
            const double eP = density(x - 1, y);
            o[0] = cp_logAdd(o[0], su[2] + (eP + t[T_GAP_OPEN_Y]));
            o[2] = cp_logAdd(o[2], su[2] + (eP + t[T_GAP_EXTEND_Y]));
        }
        const double *sl = bcell(d + 1, dTop, xmy + 1);
        if (sl) {
            o[0] = cp_logAdd(o[0], sl[1] + (GAPX_EP + t[T_GAP_OPEN_X]));
            o[1] = cp_logAdd(o[1], sl[1] + (GAPX_EP + t[T_GAP_EXTEND_X]));
            o[2] = cp_logAdd(o[2], sl[1] + (GAPX_EP + t[T_GAP_SWITCH_TO_X]));
        }
    }

    /* diagonalCalculation_Expectations :841-863 with
     * cell_signal_updateTransAndKmerSkipExpectations2 :445-476: every transition adds its posterior
     * to the transition counts; one INTO match with posterior >= the HdpHmm's threshold (carried in
     * P.threshold) also assigns the cell's event to its k-mer.  Assignments come out in the host
     * loop's order (cells by x-y, per cell from match, gapX, gapY) as (from, x-1, y-1) triples. */
    __device__ __forceinline__ void expect_diagonal(const DevGeneralArgs &a, const DevParams &P, const DevItem &it,
                                                    long long d2, int l2, int w2, const double *bdd, double total,
                                                    bool haveMiddle, long long &myPairs) {
        const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
        const double *t = model.t;
        if (tid == 0) expAcc[9] += total;
        for (int cc = tid; cc < w2; cc += 256) {
            const int xmy = l2 + 2 * cc;
            const long long x = (d2 + xmy) / 2, y = (d2 - xmy) / 2;
            const double *cur = bdd + cc * 3;
            const double *lower = fcell(d2 - 1, xmy - 1);
            const double *middle = haveMiddle ? fcell(d2 - 2, xmy) : nullptr;
            const double *upper = fcell(d2 - 1, xmy + 1);
            if (lower) {
                expAcc[0 * 3 + 1] += exp(lower[0] + cur[1] + (GAPX_EP + t[T_GAP_OPEN_X]) - total);
                expAcc[1 * 3 + 1] += exp(lower[1] + cur[1] + (GAPX_EP + t[T_GAP_EXTEND_X]) - total);
                expAcc[2 * 3 + 1] += exp(lower[2] + cur[1] + (GAPX_EP + t[T_GAP_SWITCH_TO_X]) - total);
            }
            if (middle) {
                const double eP = density(x - 1, y - 1);
                expAcc[0 * 3 + 0] += exp(middle[0] + cur[0] + (eP + t[T_MATCH_CONTINUE]) - total);
                expAcc[1 * 3 + 0] += exp(middle[1] + cur[0] + (eP + t[T_MATCH_FROM_GAP_X]) - total);
                expAcc[2 * 3 + 0] += exp(middle[2] + cur[0] + (eP + t[T_MATCH_FROM_GAP_Y]) - total);
            }
            if (upper) {
                const double eP = density(x - 1, y - 1);
                expAcc[0 * 3 + 2] += exp(upper[0] + cur[2] + (eP + t[T_GAP_OPEN_Y]) - total);
                expAcc[2 * 3 + 2] += exp(upper[2] + cur[2] + (eP + t[T_GAP_EXTEND_Y]) - total);
            }
        }
        if (wave == 0 && haveMiddle) {
            for (int base = 0; base < w2; base += 64) {
                const int cc = base + lane;
                double e[3] = { 0.0, 0.0, 0.0 };
                bool hit[3] = { false, false, false };
                long long x = 0, y = 0;
                if (cc < w2) {
                    const int xmy = l2 + 2 * cc;
                    x = (d2 + xmy) / 2;
                    y = (d2 - xmy) / 2;
                    const double *middle = fcell(d2 - 2, xmy);
                    if (middle) {
                        const double eP = density(x - 1, y - 1), cm = bdd[cc * 3];
                        e[0] = middle[0] + cm + (eP + t[T_MATCH_CONTINUE]) - total;
                        e[1] = middle[1] + cm + (eP + t[T_MATCH_FROM_GAP_X]) - total;
                        e[2] = middle[2] + cm + (eP + t[T_MATCH_FROM_GAP_Y]) - total;
#pragma unroll
                        for (int f = 0; f < 3; f++) hit[f] = exp(e[f]) >= P.threshold;
                    }
                }
                const unsigned long long below = (1ull << lane) - 1ull;
                const unsigned long long m0 = __ballot(hit[0]), m1 = __ballot(hit[1]), m2 = __ballot(hit[2]);
                long long idx = myPairs + __popcll(m0 & below) + __popcll(m1 & below) + __popcll(m2 & below);
#pragma unroll
                for (int f = 0; f < 3; f++) {
                    if (!hit[f]) continue;
                    if (idx < it.pairCap) {
                        long long *o = a.pairs + (it.pairBase + idx) * 3;
                        o[0] = f;
                        o[1] = x - 1;
                        o[2] = y - 1;
                        a.pairLogp[it.pairBase + idx] = e[f];
                    }
                    idx++;
                }
                myPairs += __popcll(m0) + __popcll(m1) + __popcll(m2);
            }
        }
    }
    /* block reduction of the per-thread partial sums, then one atomic per value */
    __device__ __forceinline__ void expect_fold(const DevGeneralArgs &a, const DevItem &it) {
        const int tid = threadIdx.x, lane = tid & 63;
        if (tid < 16) sExp[tid] = 0.0;
        __syncthreads();
        for (int i = 0; i < 10; i++) {
            double v = expAcc[i];
            for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
            if (lane == 0) atomicAdd(&sExp[i], v);
        }
        __syncthreads();
        if (tid < 10) atomicAdd(a.expect + (long long) it.model * 10 + tid, sExp[tid]);
    }
};

} // namespace

extern "C" __global__ __launch_bounds__(256) void cpecan_k_generalh(DevGeneralArgs a, DevParams P) {
    __shared__ double sExp[16];
    const DevItem it = a.items[blockIdx.x];
    Hdp m(a, it, sExp);
    general_pass(m, a, P, it);
}
