// sym_product_dump.cpp — the host builder of the multigrid hierarchy's pair-list products (toyslam_amd/csrc/host/amg.cpp: spgemm_sym) on
// caller-given patterns, without a GPU.  One case per line of stdin, one line of integers per case on stdout
// (tests/test_sym_patterns_cpu.py compares them with the reference of tests/sym_patterns.py):
//   in:   upper n ny nc has_alias xptr*(n+1) xcol*nx [x_alias*nx] yptr*(ny+1) ycol*nyz
//   out:  not_symmetric nnz pairs zptr*(n+1) zcol*nnz pl_ptr*(nnz+1) px*pairs py*pairs [mirror*nnz]          (mirror: upper = 1 only)
// Any other failure of the builder ends the program with status 1.
#include <cstdio>
#include <string>
#include <vector>

#include "host/amg.h"

using namespace tsgo;

static bool get(long long& v) { return std::scanf("%lld", &v) == 1; }
static bool get_list(std::vector<int>& out, long long n) {
    if (n < 0) return false;
    out.resize((size_t)n);
    for (int& x : out) { long long v; if (!get(v)) return false; x = (int)v; }
    return true;
}
template <typename V> static void put(const V& v) { for (int x : v) std::printf(" %d", x); }

int main() {
    long long upper, n, ny, nc, has_alias;
    while (get(upper)) {
        if (!get(n) || !get(ny) || !get(nc) || !get(has_alias) || n < 0 || ny < 0 || nc < 0) return 1;
        BlockCsr X, Y, Z;
        std::vector<int> alias, mirror;
        X.n_rows = (int)n; X.n_cols = (int)ny; Y.n_rows = (int)ny; Y.n_cols = (int)nc;
        if (!get_list(X.ptr, n + 1) || !get_list(X.col, X.ptr.back())) return 1;
        if (has_alias && !get_list(alias, X.ptr.back())) return 1;
        if (!get_list(Y.ptr, ny + 1) || !get_list(Y.col, Y.ptr.back())) return 1;
        PairList pl;
        const std::string err = spgemm_sym(X, has_alias ? &alias : nullptr, Y, Z, pl, upper ? &mirror : nullptr);
        const bool not_symmetric = err.find("not structurally symmetric") != std::string::npos;
        if (!err.empty() && !not_symmetric) { std::fprintf(stderr, "spgemm_sym: %s\n", err.c_str()); return 1; }
        std::printf("%d %d %zu", not_symmetric ? 1 : 0, Z.nnz(), pl.x.size());
        put(Z.ptr); put(Z.col); put(pl.ptr); put(pl.x); put(pl.y);
        if (upper) put(mirror);
        std::printf("\n");
    }
    return 0;
}
