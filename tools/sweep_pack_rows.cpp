// Wave-rows per chain of the CR sweep's grid at tw = 1 (csrc/gs_sweep_pack.h),
// for tools/sweep_issue_model.py.
// usage: sweep_pack_rows L   ->   "rows_plain rows_packed"
#include <cstdio>
#include <cstdlib>

#include "gs_sweep_pack.h"

int main(int argc, char** argv) {
    const int L = argc > 1 ? std::atoi(argv[1]) : 1024;
    const int tm = gs_pack::rows_per_chunk(L);
    std::printf("%lld %lld\n", gs_pack::build(L, tm, false).rows_issued, gs_pack::build(L, tm, true).rows_issued);
    return 0;
}
