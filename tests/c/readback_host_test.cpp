/* The host rules of the readback (cpecan_readback_host.h) behind a stream of cases: one case per request on stdin, its
 * result on stdout (tests/test_readback_host_cpu.py holds the expectations).  Doubles cross as hexadecimal text.
 *   v THRESHOLD E                     -> the verdict of one exponent
 *   c NT NITEMS BASE[0..NITEMS]       -> the NT + 1 cuts
 *   a N, then N x (TAG X Y E)         -> the N records in the reference's order: FROM X Y E */
#include "cpecan_readback_host.h"

#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>

static double number(std::istream &in) {
    std::string s;
    in >> s;
    return strtod(s.c_str(), nullptr);
}

int main() {
    std::string what;
    while (std::cin >> what) {
        if (what == "v") {
            const double threshold = number(std::cin), e = number(std::cin);
            printf("%d\n", settle_exponent(e, threshold));
        } else if (what == "c") {
            int nt;
            long long nItems;
            std::cin >> nt >> nItems;
            std::vector<long long> base((size_t) nItems + 1);
            for (long long &v : base) std::cin >> v;
            for (int64_t c : cut_items(base.data(), nItems, nt)) printf("%lld ", (long long) c);
            printf("\n");
        } else if (what == "a") {
            long long n;
            std::cin >> n;
            std::vector<long long> tri((size_t) n * 3);
            std::vector<double> e((size_t) n);
            for (long long k = 0; k < n; k++) {
                std::cin >> tri[(size_t) k * 3] >> tri[(size_t) k * 3 + 1] >> tri[(size_t) k * 3 + 2];
                e[(size_t) k] = number(std::cin);
            }
            order_assignments(tri.data(), e.data(), n);
            for (long long k = 0; k < n; k++)
                printf("%lld %lld %lld %a\n", tri[(size_t) k * 3], tri[(size_t) k * 3 + 1], tri[(size_t) k * 3 + 2], e[(size_t) k]);
        } else {
            fprintf(stderr, "unknown request %s\n", what.c_str());
            return 2;
        }
    }
    return 0;
}
