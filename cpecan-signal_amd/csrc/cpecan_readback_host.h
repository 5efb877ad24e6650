/*
 * cpecan_readback_host.h -- the rules of the readback (cpecan_readback.hip) that need no device: plain C++ over pointers
 * and vectors, so that a test can call them without a GPU (tests/c/readback_host_test.cpp).  Internal linkage: none of it
 * is part of the library's exports.
 */
#ifndef CPECAN_READBACK_HOST_H
#define CPECAN_READBACK_HOST_H

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

/* The verdict on one candidate from its exponent (F + B) - totalProbability: exp(), the threshold test and
 * floor(p * 1e7) with the host's libm, the one the reference calls (impl/pairwiseAligner.c:776-786).  -2: below the
 * threshold (a NaN too), otherwise the integer posterior. */
static inline int settle_exponent(double e, double threshold) {
    double p = exp(e);
    if (!(p >= threshold)) return -2;
    if (p > 1.0) p = 1.0;
    return (int) floor(p * 10000000.0);
}

/* nItems items, item i holding the candidates base[i] .. base[i + 1], cut into nt contiguous runs of about the same
 * number of candidates each: run t is the items cut[t] .. cut[t + 1] */
static inline std::vector<int64_t> cut_items(const long long *base, int64_t nItems, int nt) {
    const long long all = base[nItems];
    std::vector<int64_t> cut(1, 0);
    for (int t = 0; t < nt; t++) {
        const long long want = all * (t + 1) / nt;
        int64_t i1 = cut.back();
        while (i1 < nItems && (base[(size_t) i1 + 1] <= want || t == nt - 1)) i1++;
        cut.push_back(i1);
    }
    cut.back() = nItems;
    return cut;
}

/* The HDP machine's event assignments of one item as the wave kernels leave them: n triples p3 with their exponents pl,
 * appended by whichever thread got there, each tagged with its traceback window (first field = from-state + 4 * window).
 * The reference walks windows upwards, inside a window the diagonals downwards, a diagonal by ascending x, a cell by
 * from-state (cell_signal_updateTransAndKmerSkipExpectations2 inside diagonalCalculation_Expectations): put them so, in
 * place, the tags taken off. */
static inline void order_assignments(long long *p3, double *pl, long long n) {
    if (n <= 1) {
        if (n == 1) p3[0] &= 3;
        return;
    }
    std::vector<long long> order((size_t) n);
    for (long long k = 0; k < n; k++) order[(size_t) k] = k;
    std::sort(order.begin(), order.end(), [p3](long long a, long long c2) {
        const long long wa = p3[3 * a] >> 2, wc = p3[3 * c2] >> 2;
        if (wa != wc) return wa < wc;
        const long long da = p3[3 * a + 1] + p3[3 * a + 2], dc = p3[3 * c2 + 1] + p3[3 * c2 + 2];
        if (da != dc) return da > dc;
        if (p3[3 * a + 1] != p3[3 * c2 + 1]) return p3[3 * a + 1] < p3[3 * c2 + 1];
        return (p3[3 * a] & 3) < (p3[3 * c2] & 3);
    });
    const std::vector<long long> tri(p3, p3 + 3 * n);
    const std::vector<double> lp(pl, pl + n);
    for (long long k = 0; k < n; k++) {
        const long long src = order[(size_t) k];
        p3[3 * k] = tri[(size_t) (3 * src)] & 3;
        p3[3 * k + 1] = tri[(size_t) (3 * src + 1)];
        p3[3 * k + 2] = tri[(size_t) (3 * src + 2)];
        pl[k] = lp[(size_t) src];
    }
}

#endif
