// lazy_plan_check.cpp — stand-alone driver of lazy_plan (csrc/lazy_plan.h), built by tests/test_lazy_plan.py with the host compiler,
// plain or with the sanitizers.  One output line per leading dimension ld = 2 .. 1025:
//   ld threads mb rows shmem          (threads as launch_sweep_lazy picks them; "ld refused" where no plan fits)
#include "lazy_plan.h"
#include <cstdio>

int main()
{
    for (int ld = 2; ld <= 1025; ++ld) {
        int mb = -1, rows = -1;                      // stale contents: the function must replace them
        size_t shmem = (size_t)-1;
        if (!partls::lazy_plan(ld, &mb, &rows, &shmem)) { std::printf("%d refused\n", ld); continue; }
        std::printf("%d %d %d %d %zu\n", ld, ld <= 512 ? 512 : 1024, mb, rows, shmem);
    }
    return 0;
}
