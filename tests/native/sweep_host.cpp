// The host arithmetic of physicl_amd/csrc/pcl_sweep.h (the layer above its __HIPCC__ section) as a program of its own, for
// tests/test_sweep_cpu.py: built with g++ and the address and undefined-behaviour sanitizers, fed one question per line on
// standard input, one answer per line on standard output.  Doubles travel as C99 hex floats ("nan", "inf" as such).
//
//   grid <n_slots> <n_cu> <per_cu>     -> balanced_grid
//   lds <bytes>                        -> resident_per_cu
//   tile <length>                      -> tile_log_of
//   edges <transform> <n_bins> <e>...  -> 0, or 1 and the transformed edges
//   layout <out_bytes> <tab_bytes> <n_ids> <n_kind>   -> layout_of: tables ids kind total
//   spans <zero|copy|add> <k> <len_1> .. <len_k> <flat>...  -> cells_of, then the spans' cells after the operation.  Every
//       span is a heap array of exactly its length holding 1000 * (i + 1) + j beforehand; a span of length 0 is NULL.
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
        } else if (what == "layout") {
            unsigned long long out_bytes, tab_bytes, n_ids, n_kind;
            in >> out_bytes >> tab_bytes >> n_ids >> n_kind;
            const pcl_sweep::block_layout at = pcl_sweep::layout_of((size_t)out_bytes, (size_t)tab_bytes, (size_t)n_ids, (size_t)n_kind);
            printf("%zu %zu %zu %zu\n", at.tables, at.ids, at.kind, at.total);
        } else if (what == "spans") {
            std::string op;
            size_t k;
            in >> op >> k;
            std::vector<std::vector<int64_t>> mem(k);
            pcl_sweep::spans out;
            for (size_t i = 0; i < k; ++i) {
                size_t len;
                in >> len;
                for (size_t j = 0; j < len; ++j) mem[i].push_back((int64_t)(1000 * (i + 1) + j));
                out.push_back({len ? mem[i].data() : nullptr, len});
            }
            std::vector<int64_t> flat;       // exactly cells_of(out) values on the heap
            long long x;
            while (in >> x) flat.push_back(x);
            if (op == "zero" && flat.empty()) pcl_sweep::zero_spans(out);
            else if (op == "copy" && flat.size() == pcl_sweep::cells_of(out)) pcl_sweep::copy_to_spans(out, flat.data());
            else if (op == "add" && flat.size() == pcl_sweep::cells_of(out)) pcl_sweep::add_to_spans(out, flat.data());
            else return 2;
            printf("%zu", pcl_sweep::cells_of(out));
            for (const std::vector<int64_t> &m : mem)
                for (int64_t v : m) printf(" %lld", (long long)v);
            printf("\n");
        } else {
            return 2;
        }
    }
    return 0;
}
