/*
 * cpecan_kernel_general5.hip -- the reference's 5-state symbol machine (stateMachine5,
 * impl/stateMachine.c:829-865; BASELINE configs[0]: DNA against DNA, the reference's own CPU-runnable
 * case) on the general driver (cpecan_general.h): any band width (the un-anchored 1 kb x 1 kb case is a
 * full matrix), posterior decode and Baum-Welch expectations.  Where the widest band fits, the forward
 * sweep reads its two previous diagonals from LDS (P.ldsWidth).
 *
 * States (inc/stateMachine.h:31-35): match 0, shortGapX 1, shortGapY 2, longGapX 3, longGapY 4.
 * Backward is a gather with the reference's scatter order kept per target state: the cell on d+2
 * (its middle block), then the cell (d+1, xmy-1) (its upper block, transitions in listed order),
 * then (d+1, xmy+1) (its lower block).
 */
#include "cpecan_general.h"

/* transition slots: the order of struct _StateMachine5 (inc/stateMachine.h:108-124) */
enum {
    T5_MATCH_CONTINUE = 0, T5_MATCH_FROM_SHORT_GAP_X, T5_MATCH_FROM_LONG_GAP_X, T5_GAP_SHORT_OPEN_X,
    T5_GAP_SHORT_EXTEND_X, T5_GAP_SHORT_SWITCH_TO_X, T5_GAP_LONG_OPEN_X, T5_GAP_LONG_EXTEND_X,
    T5_GAP_LONG_SWITCH_TO_X, T5_MATCH_FROM_SHORT_GAP_Y, T5_MATCH_FROM_LONG_GAP_Y,
    T5_GAP_SHORT_OPEN_Y, T5_GAP_SHORT_EXTEND_Y, T5_GAP_SHORT_SWITCH_TO_Y, T5_GAP_LONG_OPEN_Y,
    T5_GAP_LONG_EXTEND_Y, T5_GAP_LONG_SWITCH_TO_Y
};
namespace {

/* emissions_discrete_getBaseIndex impl/stateMachine.c:104-118: anything but upper-case ACGT is "not a
 * base" (4097 there); index < 0 is the "n" sentinel of sequence_getBase (:308-312) */
__device__ __forceinline__ int base_of(const char *s, long long i) {
    if (i < 0) return 4;
    const char ch = s[i];
    return ch == 'A' ? 0 : ch == 'C' ? 1 : ch == 'G' ? 2 : ch == 'T' ? 3 : 4;
}
/* emissions_symbol_getGapProb / getMatchProb :155-173 (N-free input is a precondition, quirk Q3) */
__device__ __forceinline__ double e_gap(const double *g, int i) { return i < 4 ? g[i] : CP_NEG_INF; }
__device__ __forceinline__ double e_match(const double *m, int ix, int iy) {
    return ix < 4 && iy < 4 ? m[ix * 4 + iy] : CP_NEG_INF;
}

/* match state reached from the five states of `middle` (stateMachine5_cellCalculate :843-851) */
__device__ __forceinline__ double match_from(const double *middle, double eP, const double *t) {
    double m = CP_NEG_INF;
    m = cp_logAdd(m, middle[0] + (eP + t[T5_MATCH_CONTINUE]));
    m = cp_logAdd(m, middle[1] + (eP + t[T5_MATCH_FROM_SHORT_GAP_X]));
    m = cp_logAdd(m, middle[2] + (eP + t[T5_MATCH_FROM_SHORT_GAP_Y]));
    m = cp_logAdd(m, middle[3] + (eP + t[T5_MATCH_FROM_LONG_GAP_X]));
    m = cp_logAdd(m, middle[4] + (eP + t[T5_MATCH_FROM_LONG_GAP_Y]));
    return m;
}

/* model block: [17 transitions | pad to 24 | 16 match | 4 gapX | 4 gapY] = CP_MODEL5_STRIDE doubles */
struct Dna5 : GeneralCells<5> {
    static constexpr bool kExpect = true;
    const char *cx, *cy;    /* nucleotides of this item */
    const double *t;        /* 17 transitions */
    const double *mm;       /* 4 x 4 match emissions */
    const double *gx, *gy;  /* 4 + 4 gap emissions */
    double *ldsF; /* the forward cells of the last three diagonals, [d % 3][cell][state]; NULL: read them from HBM */
    int ldsW;
    double (*sExp)[CP_EXPECT5_LEN + 2]; /* the E-step's sums in LDS, one copy per wave */

    __device__ Dna5(const DevGeneralArgs &a, const DevItem &it, double *lds, int ldsWidth,
                    double (*sExp_)[CP_EXPECT5_LEN + 2])
        : GeneralCells<5>(a, it), ldsF(ldsWidth > 0 ? lds : nullptr), ldsW(ldsWidth), sExp(sExp_) {
        cx = (const char *) a.x + it.xOff;
        cy = (const char *) a.y + it.yOff;
        const double *model = (const double *) a.models + (long long) it.model * CP_MODEL5_STRIDE;
        t = model;
        mm = model + 24;
        gx = model + 40;
        gy = model + 44;
    }

    __device__ __forceinline__ double *lds_diagonal(long long d) const {
        return ldsF ? ldsF + (d % 3) * (long long) ldsW * S : nullptr;
    }
    /* fcell for the forward sweep's own neighbours (diagonals d - 1 and d - 2 of the diagonal being computed) */
    __device__ __forceinline__ const double *fcell_sweep(long long d, int xmy) const {
        if (d < 0) return nullptr;
        const int l = L[d], r = R[d];
        if (xmy < l || xmy > r) return nullptr;
        if (ldsF) return ldsF + ((d % 3) * (long long) ldsW + ((xmy - l) >> 1)) * S;
        return F + (pre[d] + ((xmy - l) >> 1)) * S;
    }
    __device__ __forceinline__ double match_into(const double *middle, long long x, long long y) const {
        return match_from(middle, e_match(mm, base_of(cx, x - 1), base_of(cy, y - 1)), t);
    }

    /* stateMachine5_startStateProb / raggedStartStateProb (:743-763) */
    __device__ __forceinline__ void start_vector(bool ragged, double e[S]) const {
        e[0] = ragged ? CP_NEG_INF : 0.0;
        e[1] = CP_NEG_INF;
        e[2] = CP_NEG_INF;
        e[3] = ragged ? 0.0 : CP_NEG_INF;
        e[4] = ragged ? 0.0 : CP_NEG_INF;
    }
    /* stateMachine5_endStateProb / raggedEndStateProb (:765-789) */
    __device__ __forceinline__ void end_vector(bool ragged, double e[S]) const {
        if (ragged) {
            e[0] = t[T5_GAP_LONG_OPEN_X];
            e[1] = t[T5_GAP_LONG_OPEN_X];
            e[2] = t[T5_GAP_LONG_OPEN_Y];
            e[3] = t[T5_GAP_LONG_EXTEND_X];
            e[4] = t[T5_GAP_LONG_EXTEND_Y];
        } else {
            e[0] = t[T5_MATCH_CONTINUE];
            e[1] = t[T5_MATCH_FROM_SHORT_GAP_X];
            e[2] = t[T5_MATCH_FROM_SHORT_GAP_Y];
            e[3] = t[T5_MATCH_FROM_LONG_GAP_X];
            e[4] = t[T5_MATCH_FROM_LONG_GAP_Y];
        }
    }

    /* cell_calculateForward (:365-376) over stateMachine5_cellCalculate (:829-865) */
    __device__ __forceinline__ void forward_cell(long long d, int xmy, double o[S]) const {
        const long long x = (d + xmy) / 2, y = (d - xmy) / 2;
        const int bx = base_of(cx, x - 1), by = base_of(cy, y - 1);
#pragma unroll
        for (int s = 0; s < S; s++) o[s] = CP_NEG_INF;
        const double *lower = fcell_sweep(d - 1, xmy - 1);
        const double *middle = fcell_sweep(d - 2, xmy);
        const double *upper = fcell_sweep(d - 1, xmy + 1);
        if (lower) {
            const double eP = e_gap(gx, bx);
            o[1] = cp_logAdd(o[1], lower[0] + (eP + t[T5_GAP_SHORT_OPEN_X]));
            o[1] = cp_logAdd(o[1], lower[1] + (eP + t[T5_GAP_SHORT_EXTEND_X]));
            o[3] = cp_logAdd(o[3], lower[0] + (eP + t[T5_GAP_LONG_OPEN_X]));
            o[3] = cp_logAdd(o[3], lower[3] + (eP + t[T5_GAP_LONG_EXTEND_X]));
        }
        if (middle) o[0] = match_from(middle, e_match(mm, bx, by), t);
        if (upper) {
            const double eP = e_gap(gy, by);
            o[2] = cp_logAdd(o[2], upper[0] + (eP + t[T5_GAP_SHORT_OPEN_Y]));
            o[2] = cp_logAdd(o[2], upper[2] + (eP + t[T5_GAP_SHORT_EXTEND_Y]));
            o[4] = cp_logAdd(o[4], upper[0] + (eP + t[T5_GAP_LONG_OPEN_Y]));
            o[4] = cp_logAdd(o[4], upper[4] + (eP + t[T5_GAP_LONG_EXTEND_Y]));
        }
    }

    /* gather form of cell_calculateBackward (:378-389) */
    __device__ __forceinline__ void backward_cell(long long d, long long dTop, int xmy, double o[S]) const {
        const long long x = (d + xmy) / 2, y = (d - xmy) / 2;
#pragma unroll
        for (int s = 0; s < S; s++) o[s] = CP_NEG_INF;
        /* (ii) cell (x+1, y+1) on d+2 reaches this cell through its middle block */
        const double *s2 = bcell(d + 2, dTop, xmy);
        if (s2) {
            const double eP = e_match(mm, base_of(cx, x), base_of(cy, y));
            o[0] = cp_logAdd(o[0], s2[0] + (eP + t[T5_MATCH_CONTINUE]));
            o[1] = cp_logAdd(o[1], s2[0] + (eP + t[T5_MATCH_FROM_SHORT_GAP_X]));
            o[2] = cp_logAdd(o[2], s2[0] + (eP + t[T5_MATCH_FROM_SHORT_GAP_Y]));
            o[3] = cp_logAdd(o[3], s2[0] + (eP + t[T5_MATCH_FROM_LONG_GAP_X]));
            o[4] = cp_logAdd(o[4], s2[0] + (eP + t[T5_MATCH_FROM_LONG_GAP_Y]));
        }
        /* (iii) cell (x, y+1) on d+1 reaches it through its upper block */
        const double *su = bcell(d + 1, dTop, xmy - 1);
        if (su) {
            const double eP = e_gap(gy, base_of(cy, y));
            o[0] = cp_logAdd(o[0], su[2] + (eP + t[T5_GAP_SHORT_OPEN_Y]));
            o[2] = cp_logAdd(o[2], su[2] + (eP + t[T5_GAP_SHORT_EXTEND_Y]));
            o[0] = cp_logAdd(o[0], su[4] + (eP + t[T5_GAP_LONG_OPEN_Y]));
            o[4] = cp_logAdd(o[4], su[4] + (eP + t[T5_GAP_LONG_EXTEND_Y]));
        }
        /* (iv) cell (x+1, y) on d+1 reaches it through its lower block */
        const double *sl = bcell(d + 1, dTop, xmy + 1);
        if (sl) {
            const double eP = e_gap(gx, base_of(cx, x));
            o[0] = cp_logAdd(o[0], sl[1] + (eP + t[T5_GAP_SHORT_OPEN_X]));
            o[1] = cp_logAdd(o[1], sl[1] + (eP + t[T5_GAP_SHORT_EXTEND_X]));
            o[0] = cp_logAdd(o[0], sl[3] + (eP + t[T5_GAP_LONG_OPEN_X]));
            o[3] = cp_logAdd(o[3], sl[3] + (eP + t[T5_GAP_LONG_EXTEND_X]));
        }
    }

    /* diagonalCalculation_Expectations :841-863 over stateMachine5_cellCalculate with
     * cell_updateExpectations (:407-424): every transition into a cell of backward[d2] from its
     * forward neighbours adds p = exp(from + to + (eP + tP) - total) to its transition count and,
     * unless a base is not ACGT, to the emission count [to][x][y] */
    __device__ __forceinline__ void expect_diagonal(const DevGeneralArgs &, const DevParams &, const DevItem &,
                                                    long long d2, int l2, int w2, const double *bdd, double total,
                                                    bool haveMiddle, long long &) const {
        const int tid = threadIdx.x, wave = tid >> 6;
        double *acc = sExp[wave];
        if (tid == 0) acc[CP_EXPECT5_LEN - 1] += total; /* likelihood, once per diagonal (quirk Q7) */
        for (int cc = tid; cc < w2; cc += 256) {
            const int xmy = l2 + 2 * cc;
            const long long x = (d2 + xmy) / 2, y = (d2 - xmy) / 2;
            const int bx = base_of(cx, x - 1), by = base_of(cy, y - 1);
            const double *cur = bdd + cc * S;
            const double *lower = fcell(d2 - 1, xmy - 1);
            const double *middle = haveMiddle ? fcell(d2 - 2, xmy) : nullptr;
            const double *upper = fcell(d2 - 1, xmy + 1);
            double into[S] = { 0.0, 0.0, 0.0, 0.0, 0.0 }; /* per to-state sums for the emission counts */
            auto tr = [&](const double *nb, int f, int to, double eP, int ti) {
                const double pr = exp(nb[f] + cur[to] + (eP + t[ti]) - total);
                atomicAdd(&acc[f * S + to], pr);
                into[to] += pr;
            };
            if (lower) {
                const double eP = e_gap(gx, bx);
                tr(lower, 0, 1, eP, T5_GAP_SHORT_OPEN_X);
                tr(lower, 1, 1, eP, T5_GAP_SHORT_EXTEND_X);
                tr(lower, 0, 3, eP, T5_GAP_LONG_OPEN_X);
                tr(lower, 3, 3, eP, T5_GAP_LONG_EXTEND_X);
            }
            if (middle) {
                const double eP = e_match(mm, bx, by);
                tr(middle, 0, 0, eP, T5_MATCH_CONTINUE);
                tr(middle, 1, 0, eP, T5_MATCH_FROM_SHORT_GAP_X);
                tr(middle, 2, 0, eP, T5_MATCH_FROM_SHORT_GAP_Y);
                tr(middle, 3, 0, eP, T5_MATCH_FROM_LONG_GAP_X);
                tr(middle, 4, 0, eP, T5_MATCH_FROM_LONG_GAP_Y);
            }
            if (upper) {
                const double eP = e_gap(gy, by);
                tr(upper, 0, 2, eP, T5_GAP_SHORT_OPEN_Y);
                tr(upper, 2, 2, eP, T5_GAP_SHORT_EXTEND_Y);
                tr(upper, 0, 4, eP, T5_GAP_LONG_OPEN_Y);
                tr(upper, 4, 4, eP, T5_GAP_LONG_EXTEND_Y);
            }
            if (bx < 4 && by < 4) {
#pragma unroll
                for (int st = 0; st < S; st++)
                    if (into[st] != 0.0) atomicAdd(&acc[25 + st * 16 + bx * 4 + by], into[st]);
            }
        }
    }
    __device__ __forceinline__ void expect_fold(const DevGeneralArgs &a, const DevItem &it) const {
        __syncthreads();
        double *dst = a.expect + (long long) it.model * CP_EXPECT5_LEN;
        for (int i = threadIdx.x; i < CP_EXPECT5_LEN; i += 256) {
            const double v = ((sExp[0][i] + sExp[1][i]) + sExp[2][i]) + sExp[3][i];
            if (v != 0.0) atomicAdd(dst + i, v);
        }
    }
};

} // namespace

extern "C" __global__ __launch_bounds__(256) void cpecan_k_general5(DevGeneralArgs a, DevParams P) {
    extern __shared__ double ldsDiagonals[]; /* the last three forward diagonals, P.ldsWidth cells each (launch-time size) */
    /* Baum-Welch sums of this alignment: 25 transitions [from*5+to], 80 emissions [state*16+x*4+y] and the
     * likelihood, one copy per wave (LDS atomics), folded into the model's block of `expect` at the end */
    __shared__ double sExp[4][CP_EXPECT5_LEN + 2];
    for (int i = threadIdx.x; i < 4 * (CP_EXPECT5_LEN + 2); i += 256) (&sExp[0][0])[i] = 0.0;
    const DevItem it = a.items[blockIdx.x];
    Dna5 m(a, it, ldsDiagonals, P.ldsWidth, sExp);
    general_pass(m, a, P, it);
}
