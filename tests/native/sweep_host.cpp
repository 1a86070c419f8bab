// The host arithmetic of physicl_amd/csrc/pcl_sweep.h (the layer above its __HIPCC__ section) as a program of its own, for
// tests/test_sweep_cpu.py: built with g++ and the address and undefined-behaviour sanitizers, fed one question per line on
// standard input, one answer per line on standard output.  Doubles travel as C99 hex floats ("nan", "inf" as such).
//
//   grid <n_slots> <n_cu> <per_cu>     -> balanced_grid
//   lds <bytes>                        -> resident_per_cu
//   tile <length>                      -> tile_log_of
//   edges <transform> <n_bins> <e>...  -> 0, or 1 and the transformed edges
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "pcl_sweep.h"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        in >> what;
        if (what == "grid") {
            long long n_slots;
            int n_cu, per_cu;
            in >> n_slots >> n_cu >> per_cu;
            printf("%lld\n", (long long)pcl_sweep::balanced_grid(n_slots, n_cu, per_cu));
        } else if (what == "lds") {
            unsigned long long bytes;
            in >> bytes;
            printf("%d\n", pcl_sweep::resident_per_cu((size_t)bytes));
        } else if (what == "tile") {
            long long tile;
            in >> tile;
            printf("%d\n", pcl_sweep::tile_log_of(tile));
        } else if (what == "edges") {
            int t, n_bins;
            in >> t >> n_bins;
            std::vector<double> e, to;       // exactly n_bins + 1 doubles on the heap: a read past them is the sanitizer's
            std::string tok;
            while (in >> tok) e.push_back(strtod(tok.c_str(), nullptr));
            if ((int)e.size() != n_bins + 1) return 2;
            const bool ok = pcl_sweep::check_edges(e.data(), n_bins, (pcl_sweep::edge_transform)t, &to);
            if (ok != pcl_sweep::check_edges(e.data(), n_bins, (pcl_sweep::edge_transform)t)) return 3; // (with and without a vector)
            printf("%d", ok ? 1 : 0);
            if (ok)
                for (double v : to) printf(" %a", v);
            printf("\n");
        } else {
            return 2;
        }
    }
    return 0;
}
