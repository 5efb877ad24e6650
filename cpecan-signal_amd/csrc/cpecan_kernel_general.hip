/*
 * cpecan_kernel_general.hip -- the strawMan signal machine (stateMachine3, impl/stateMachine.c:1305-1334) on the
 * general driver (cpecan_general.h): bands of any width, posterior decode, Baum-Welch expectations and cell dumps.
 */
#include "cpecan_general.h"

namespace {

/* emissions_signal_strawManGetKmerEventMatchProb impl/stateMachine.c:595-629 */
__device__ __forceinline__ double emit_match(const double *r, double mean, double noise) {
    double a = cp_logGauss(mean, r[CP_MU], r[CP_SD], r[CP_K1]);
    double b = cp_logGauss(noise, r[CP_NMU], r[CP_NSD], r[CP_K2]);
    return a + b;
}
__device__ __forceinline__ double emit_gapy(const double *r, double mean, double noise) {
    double a = cp_logGauss(mean, r[CP_YMU], r[CP_YSD], r[CP_YK1]);
    double b = cp_logGauss(noise, r[CP_YNMU], r[CP_YNSD], r[CP_YK2]);
    return a + b;
}

struct StrawMan : GeneralCells<3> {
    static constexpr bool kExpect = true;
    static constexpr bool kDump = true;
    const unsigned short *kidx;  /* k-mer index per X element (0..4095, 4096 = invalid) */
    const double *ev;            /* events of this item, 3 doubles each */
    const double *rows;          /* model rows */
    const double *t;             /* 9 transitions */
    double expAcc[10];           /* per-thread partial expectations: 9 transitions + likelihood */
    double *gapAcc;              /* the model's gap-X expectations per k-mer */
    double *sExp;                /* [16] in LDS: the block reduction of expAcc */

    __device__ StrawMan(const DevGeneralArgs &a, const DevItem &it, double *sExp_) : GeneralCells<3>(a, it), sExp(sExp_) {
        kidx = (const unsigned short *) a.x + it.xOff;
        ev = (const double *) a.y + 3 * it.yOff;
        const double *model = (const double *) a.models + (long long) it.model * CP_MODEL_STRIDE;
        t = model;
        rows = model + CP_MODEL_HEADER;
        for (int i = 0; i < 10; i++) expAcc[i] = 0.0;
        gapAcc = a.expect ? a.expect + (long long) it.model * (9 + 4096 + 1) + 9 : nullptr;
    }

    __device__ __forceinline__ const double *row_of(long long ix) const {
        /* X element ix-1 ... caller passes the sequence index; index < 0 is the "n" sentinel (:314-318) */
        int k = ix >= 0 ? (int) kidx[ix] : 4096;
        return rows + (long long) k * CP_ROW;
    }
    __device__ __forceinline__ void event_of(long long iy, double &mean, double &noise) const {
        /* index < 0 is NULLEVENT = {-inf, 0} (:261,:333-337) */
        if (iy >= 0) {
            mean = ev[3 * iy];
            noise = ev[3 * iy + 1];
        } else {
            mean = CP_NEG_INF;
            noise = 0.0;
        }
    }
    __device__ __forceinline__ double match_from(const double *middle, double eP) const {
        double m = CP_NEG_INF;
        m = cp_logAdd(m, middle[0] + (eP + t[T_MATCH_CONTINUE]));
        m = cp_logAdd(m, middle[1] + (eP + t[T_MATCH_FROM_GAP_X]));
        m = cp_logAdd(m, middle[2] + (eP + t[T_MATCH_FROM_GAP_Y]));
        return m;
    }
    __device__ __forceinline__ double match_into(const double *middle, long long x, long long y) const {
        double mean, noise;
        event_of(y - 1, mean, noise);
        return match_from(middle, emit_match(row_of(x - 1), mean, noise));
    }

    /* stateMachine3_startStateProb / raggedStartStateProb :1168-1177 */
    __device__ __forceinline__ void start_vector(bool ragged, double e[3]) const {
        e[0] = ragged ? CP_NEG_INF : 0.0;
        e[1] = ragged ? 0.0 : CP_NEG_INF;
        e[2] = ragged ? 0.0 : CP_NEG_INF;
    }
    /* stateMachine3_endStateProb / raggedEndStateProb :1179-1207 */
    __device__ __forceinline__ void end_vector(bool ragged, double e[3]) const {
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

    /* forward cell: cell_calculateForward + stateMachine3_cellCalculate (impl/stateMachine.c:1305-1334) */
    __device__ __forceinline__ void forward_cell(long long d, int xmy, double out[3]) const {
        long long x = (d + xmy) / 2, y = (d - xmy) / 2;
        const double *row = row_of(x - 1);
        double mean, noise;
        event_of(y - 1, mean, noise);
        double m = CP_NEG_INF, gx = CP_NEG_INF, gy = CP_NEG_INF;
        const double *lower = fcell(d - 1, xmy - 1);
        const double *middle = fcell(d - 2, xmy);
        const double *upper = fcell(d - 1, xmy + 1);
        if (lower) {
            double eP = row[CP_GAPX];
            gx = cp_logAdd(gx, lower[0] + (eP + t[T_GAP_OPEN_X]));
            gx = cp_logAdd(gx, lower[1] + (eP + t[T_GAP_EXTEND_X]));
            gx = cp_logAdd(gx, lower[2] + (eP + t[T_GAP_SWITCH_TO_X]));
        }
        if (middle) m = match_from(middle, emit_match(row, mean, noise));
        if (upper) {
            double eP = emit_gapy(row, mean, noise);
            gy = cp_logAdd(gy, upper[0] + (eP + t[T_GAP_OPEN_Y]));
            gy = cp_logAdd(gy, upper[2] + (eP + t[T_GAP_EXTEND_Y]));
        }
        out[0] = m; out[1] = gx; out[2] = gy;
    }

    /* backward cell, gather form of cell_calculateBackward (:378-389) */
    __device__ __forceinline__ void backward_cell(long long d, long long dTop, int xmy, double out[3]) const {
        long long x = (d + xmy) / 2, y = (d - xmy) / 2;
        double m = CP_NEG_INF, gx = CP_NEG_INF, gy = CP_NEG_INF;
        /* (ii) cell (x+1,y+1) on d+2 reaches this cell through its middle block */
        const double *s2 = bcell(d + 2, dTop, xmy);
        if (s2) {
            const double *row = row_of(x);
            double mean, noise;
            event_of(y, mean, noise);
            double eP = emit_match(row, mean, noise);
            m = cp_logAdd(m, s2[0] + (eP + t[T_MATCH_CONTINUE]));
            gx = cp_logAdd(gx, s2[0] + (eP + t[T_MATCH_FROM_GAP_X]));
            gy = cp_logAdd(gy, s2[0] + (eP + t[T_MATCH_FROM_GAP_Y]));
        }
        /* (iii) cell (x,y+1) on d+1 reaches it through its upper block */
        const double *su = bcell(d + 1, dTop, xmy - 1);
        if (su) {
            const double *row = row_of(x - 1);
            double mean, noise;
            event_of(y, mean, noise);
            double eP = emit_gapy(row, mean, noise);
            m = cp_logAdd(m, su[2] + (eP + t[T_GAP_OPEN_Y]));
            gy = cp_logAdd(gy, su[2] + (eP + t[T_GAP_EXTEND_Y]));
        }
        /* (iv) cell (x+1,y) on d+1 reaches it through its lower block */
        const double *sl = bcell(d + 1, dTop, xmy + 1);
        if (sl) {
            const double *row = row_of(x);
            double eP = row[CP_GAPX];
            m = cp_logAdd(m, sl[1] + (eP + t[T_GAP_OPEN_X]));
            gx = cp_logAdd(gx, sl[1] + (eP + t[T_GAP_EXTEND_X]));
            gy = cp_logAdd(gy, sl[1] + (eP + t[T_GAP_SWITCH_TO_X]));
        }
        out[0] = m; out[1] = gx; out[2] = gy;
    }

    /* diagonalCalculation_Expectations :841-863 with cell_signal_updateTransAndKmerSkipExpectations :426-443 */
    __device__ __forceinline__ void expect_diagonal(const DevGeneralArgs &, const DevParams &, const DevItem &,
                                                    long long d2, int l2, int w2, const double *bdd, double total,
                                                    bool haveMiddle, long long &) {
        const int tid = threadIdx.x;
        if (tid == 0) expAcc[9] += total;
        for (int cc = tid; cc < w2; cc += 256) {
            int xmy = l2 + 2 * cc;
            long long x = (d2 + xmy) / 2, y = (d2 - xmy) / 2;
            const double *cur = bdd + cc * 3;
            const double *row = row_of(x - 1);
            double mean, noise;
            event_of(y - 1, mean, noise);
            const double *lower = fcell(d2 - 1, xmy - 1);
            const double *middle = haveMiddle ? fcell(d2 - 2, xmy) : nullptr;
            const double *upper = fcell(d2 - 1, xmy + 1);
            if (lower) {
                double eP = row[CP_GAPX];
                double p0 = exp(lower[0] + cur[1] + (eP + t[T_GAP_OPEN_X]) - total);
                double p1 = exp(lower[1] + cur[1] + (eP + t[T_GAP_EXTEND_X]) - total);
                double p2 = exp(lower[2] + cur[1] + (eP + t[T_GAP_SWITCH_TO_X]) - total);
                expAcc[0 * 3 + 1] += p0;
                expAcc[1 * 3 + 1] += p1;
                expAcc[2 * 3 + 1] += p2;
                int k = x - 1 >= 0 ? (int) kidx[x - 1] : 4096;
                if (k < 4096 && gapAcc) {
                    atomicAdd(gapAcc + k, p0);
                    atomicAdd(gapAcc + k, p1);
                    atomicAdd(gapAcc + k, p2);
                }
            }
            if (middle) {
                double eP = emit_match(row, mean, noise);
                expAcc[0 * 3 + 0] += exp(middle[0] + cur[0] + (eP + t[T_MATCH_CONTINUE]) - total);
                expAcc[1 * 3 + 0] += exp(middle[1] + cur[0] + (eP + t[T_MATCH_FROM_GAP_X]) - total);
                expAcc[2 * 3 + 0] += exp(middle[2] + cur[0] + (eP + t[T_MATCH_FROM_GAP_Y]) - total);
            }
            if (upper) {
                double eP = emit_gapy(row, mean, noise);
                expAcc[0 * 3 + 2] += exp(upper[0] + cur[2] + (eP + t[T_GAP_OPEN_Y]) - total);
                expAcc[2 * 3 + 2] += exp(upper[2] + cur[2] + (eP + t[T_GAP_EXTEND_Y]) - total);
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
        double *dst = a.expect + (long long) it.model * (9 + 4096 + 1);
        if (tid < 9) atomicAdd(dst + tid, sExp[tid]);
        if (tid == 9) atomicAdd(dst + 9 + 4096, sExp[9]);
    }
};

} // namespace

extern "C" __global__ __launch_bounds__(256) void cpecan_k_general(DevGeneralArgs a, DevParams P) {
    __shared__ double sExp[16];
    const DevItem it = a.items[blockIdx.x];
    StrawMan m(a, it, sExp);
    general_pass(m, a, P, it);
}
