/*
 * cpecan_kernel_general4.hip -- banded forward / backward / posterior DP for the reference's 4-state signal machine
 * (stateMachine4_cellCalculate, impl/stateMachine.c:867-897; getStateMachine4 :1750-1759; vanillaAlign.c:122-123):
 * match, short gap X, short gap Y and a long gap X over the strawMan emissions -- the k-mer / event Gaussian pair for
 * a match and, with the extra-event table, for a gap in Y; the k-mer gap table for a gap in X.
 *
 * On the general driver (cpecan_general.h): any band width; the backward recurrence is the gather form of the
 * reference's scatter, contributions added in the reference's order per target state.  Posterior decode only: the
 * reference has no Hmm container for this machine
 * (hmmContinuous_getEmptyHmm, impl/continuousHmm.c:913-945, knows threeState, threeStateHdp and vanilla).
 *
 * The model is a strawMan table (cpecan_models.hip: derive_rows) whose header holds the machine's eleven transitions in the
 * member order of _StateMachine4 (inc/stateMachine.h:134-152).
 */
#include "cpecan_general.h"

namespace {

enum { /* _StateMachine4's members in order */
    T4_MATCH_CONTINUE = 0, T4_MATCH_FROM_SHORT_GAP_X, T4_MATCH_FROM_LONG_GAP_X, T4_MATCH_FROM_SHORT_GAP_Y,
    T4_GAP_SHORT_OPEN_X, T4_GAP_SHORT_EXTEND_X, T4_GAP_SHORT_OPEN_Y, T4_GAP_SHORT_EXTEND_Y,
    T4_GAP_LONG_OPEN_X, T4_GAP_LONG_EXTEND_X, T4_GAP_LONG_SWITCH_TO_X
};
/* emissions_signal_strawManGetKmerEventMatchProb (impl/stateMachine.c:595-629) over the match / extra-event table */
__device__ __forceinline__ double emitM4(const double *r, double mean, double noise) {
    return cp_logGauss(mean, r[CP_MU], r[CP_SD], r[CP_K1]) + cp_logGauss(noise, r[CP_NMU], r[CP_NSD], r[CP_K2]);
}
__device__ __forceinline__ double emitY4(const double *r, double mean, double noise) {
    return cp_logGauss(mean, r[CP_YMU], r[CP_YSD], r[CP_YK1]) + cp_logGauss(noise, r[CP_YNMU], r[CP_YNSD], r[CP_YK2]);
}

/* states (inc/stateMachine.h:31-33): match 0, shortGapX 1, shortGapY 2, longGapX 3 */
struct Sm4 : GeneralCells<4> {
    const unsigned short *kidx;
    const double *ev;
    const double *rows;
    const double *t;

    __device__ Sm4(const DevGeneralArgs &a, const DevItem &it) : GeneralCells<4>(a, it) {
        kidx = (const unsigned short *) a.x + it.xOff;
        ev = (const double *) a.y + 3 * it.yOff;
        const double *model = (const double *) a.models + (long long) it.model * CP_MODEL_STRIDE;
        t = model;
        rows = model + CP_MODEL_HEADER;
    }

    __device__ __forceinline__ const double *row4(long long ix) const {
        const int k = ix >= 0 ? (int) kidx[ix] : 4096; /* index < 0: the "n" sentinel (impl/pairwiseAligner.c:314-318) */
        return rows + (long long) k * CP_ROW;
    }
    __device__ __forceinline__ void event4(long long iy, double &mean, double &noise) const {
        if (iy >= 0) { mean = ev[3 * iy]; noise = ev[3 * iy + 1]; }
        else { mean = CP_NEG_INF; noise = 0.0; } /* NULLEVENT (:261) */
    }
    /* the match state's incoming sum from the cell (x-1, y-1): the middle block of stateMachine4_cellCalculate (:884-890) */
    __device__ __forceinline__ double match_from4(const double *middle, double eP) const {
        double m = CP_NEG_INF;
        m = cp_logAdd(m, middle[0] + (eP + t[T4_MATCH_CONTINUE]));
        m = cp_logAdd(m, middle[1] + (eP + t[T4_MATCH_FROM_SHORT_GAP_X]));
        m = cp_logAdd(m, middle[2] + (eP + t[T4_MATCH_FROM_SHORT_GAP_Y]));
        m = cp_logAdd(m, middle[3] + (eP + t[T4_MATCH_FROM_LONG_GAP_X]));
        return m;
    }
    __device__ __forceinline__ double match_into(const double *middle, long long x, long long y) const {
        double mean, noise;
        event4(y - 1, mean, noise);
        return match_from4(middle, emitM4(row4(x - 1), mean, noise));
    }

    /* stateMachine5_startStateProb / stateMachine4_raggedStartStateProb (:743, :791) */
    __device__ __forceinline__ void start_vector(bool ragged, double e[S]) const {
        e[0] = ragged ? CP_NEG_INF : 0.0;
        e[1] = CP_NEG_INF;
        e[2] = ragged ? 0.0 : CP_NEG_INF;
        e[3] = ragged ? 0.0 : CP_NEG_INF;
    }
    /* stateMachine4_endStateProb / _raggedEndStateProb (:796-829) */
    __device__ __forceinline__ void end_vector(bool ragged, double e[S]) const {
        if (ragged) {
            e[0] = e[1] = e[2] = t[T4_GAP_LONG_OPEN_X];
            e[3] = t[T4_GAP_LONG_EXTEND_X];
        } else {
            e[0] = t[T4_MATCH_CONTINUE];
            e[1] = t[T4_MATCH_FROM_SHORT_GAP_X];
            e[2] = t[T4_MATCH_FROM_SHORT_GAP_Y];
            e[3] = t[T4_MATCH_FROM_LONG_GAP_X];
        }
    }

    /* cell_calculateForward (impl/pairwiseAligner.c:365-375) over stateMachine4_cellCalculate */
    __device__ __forceinline__ void forward_cell(long long d, int xmy, double o[S]) const {
        const long long x = (d + xmy) / 2, y = (d - xmy) / 2;
        const double *row = row4(x - 1);
        double mean, noise;
        event4(y - 1, mean, noise);
        double m = CP_NEG_INF, sx = CP_NEG_INF, sy = CP_NEG_INF, lx = CP_NEG_INF;
        const double *lower = fcell(d - 1, xmy - 1), *middle = fcell(d - 2, xmy), *upper = fcell(d - 1, xmy + 1);
        if (lower) {
            const double eP = row[CP_GAPX];
            sx = cp_logAdd(sx, lower[0] + (eP + t[T4_GAP_SHORT_OPEN_X]));
            sx = cp_logAdd(sx, lower[1] + (eP + t[T4_GAP_SHORT_EXTEND_X]));
            lx = cp_logAdd(lx, lower[0] + (eP + t[T4_GAP_LONG_OPEN_X]));
            lx = cp_logAdd(lx, lower[3] + (eP + t[T4_GAP_LONG_EXTEND_X]));
            lx = cp_logAdd(lx, lower[2] + (eP + t[T4_GAP_LONG_SWITCH_TO_X]));
        }
        if (middle) m = match_from4(middle, emitM4(row, mean, noise));
        if (upper) {
            const double eP = emitY4(row, mean, noise);
            sy = cp_logAdd(sy, upper[0] + (eP + t[T4_GAP_SHORT_OPEN_Y]));
            sy = cp_logAdd(sy, upper[2] + (eP + t[T4_GAP_SHORT_EXTEND_Y]));
        }
        o[0] = m; o[1] = sx; o[2] = sy; o[3] = lx;
    }

    /* gather form of cell_calculateBackward (:378-389): what reaches this cell from the cell above-right on d+2 (its
     * middle block), from (x, y+1) on d+1 (its upper block) and from (x+1, y) on d+1 (its lower block), in that order;
     * within a block in the order of stateMachine4_cellCalculate's calls */
    __device__ __forceinline__ void backward_cell(long long d, long long dTop, int xmy, double o[S]) const {
        const long long x = (d + xmy) / 2, y = (d - xmy) / 2;
        double m = CP_NEG_INF, sx = CP_NEG_INF, sy = CP_NEG_INF, lx = CP_NEG_INF;
        const double *s2 = bcell(d + 2, dTop, xmy);
        if (s2) {
            double mean, noise;
            event4(y, mean, noise);
            const double eP = emitM4(row4(x), mean, noise);
            m = cp_logAdd(m, s2[0] + (eP + t[T4_MATCH_CONTINUE]));
            sx = cp_logAdd(sx, s2[0] + (eP + t[T4_MATCH_FROM_SHORT_GAP_X]));
            sy = cp_logAdd(sy, s2[0] + (eP + t[T4_MATCH_FROM_SHORT_GAP_Y]));
            lx = cp_logAdd(lx, s2[0] + (eP + t[T4_MATCH_FROM_LONG_GAP_X]));
        }
        const double *su = bcell(d + 1, dTop, xmy - 1);
        if (su) {
            double mean, noise;
            event4(y, mean, noise);
            const double eP = emitY4(row4(x - 1), mean, noise);
            m = cp_logAdd(m, su[2] + (eP + t[T4_GAP_SHORT_OPEN_Y]));
            sy = cp_logAdd(sy, su[2] + (eP + t[T4_GAP_SHORT_EXTEND_Y]));
        }
        const double *sl = bcell(d + 1, dTop, xmy + 1);
        if (sl) {
            const double eP = row4(x)[CP_GAPX];
            m = cp_logAdd(m, sl[1] + (eP + t[T4_GAP_SHORT_OPEN_X]));
            sx = cp_logAdd(sx, sl[1] + (eP + t[T4_GAP_SHORT_EXTEND_X]));
            m = cp_logAdd(m, sl[3] + (eP + t[T4_GAP_LONG_OPEN_X]));
            lx = cp_logAdd(lx, sl[3] + (eP + t[T4_GAP_LONG_EXTEND_X]));
            sy = cp_logAdd(sy, sl[3] + (eP + t[T4_GAP_LONG_SWITCH_TO_X]));
        }
        o[0] = m; o[1] = sx; o[2] = sy; o[3] = lx;
    }
};

} // namespace

extern "C" __global__ __launch_bounds__(256) void cpecan_k_general4(DevGeneralArgs a, DevParams P) {
    const DevItem it = a.items[blockIdx.x];
    Sm4 m(a, it);
    general_pass(m, a, P, it);
}
