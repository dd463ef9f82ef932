// lazy_plan.h — the LDS plan of the deferred-update sweep kernel (sweep_lazy.hip), host only: nothing from HIP is included, so the
// function also builds with a plain host compiler (tests/native/lazy_plan_check.cpp prints it for every ld; tests/test_lazy_plan.py
// holds it against the Python restatement that tests/test_gpu_lazy_plans.py draws its table of cases from).
// The two constants are copies; sweep_lazy.hip ties them to GJ_MB (gj_panel.h) and LZ_MT with static_asserts.
#pragma once
#include <cstddef>

namespace partls {

static constexpr int LAZY_PLAN_MB = 16;     // == GJ_MB: pivots per block at most
static constexpr int LAZY_PLAN_MT = 8;      // == LZ_MT: the compiled panel width of the 1024-thread plan
static constexpr int LZ_MAXR = 64;          // rows of the LDS pool at most

// LDS plan for leading dimension ld: pivots per block and rows of the pool (pending terms + panel).  false: no plan fits (never for n <= 1023)
inline bool lazy_plan(int ld, int *mb_out, int *rows_out, size_t *shmem_out)
{
    constexpr int GJ_MB = LAZY_PLAN_MB, LZ_MT = LAZY_PLAN_MT;
    const size_t budget = (size_t)151 * 1024;
    const size_t fixed = (size_t)ld * 8 /* qs */ + 4 * (size_t)ld * 8 /* read-ahead rows */ + 3 * (size_t)ld /* flags, rowj */ + (2 * GJ_MB * GJ_MB + 8 * GJ_MB + 18) * 8 + 64;
    const size_t row = (size_t)ld * 8;
    if (budget < fixed + 6 * (row + 8 + GJ_MB * 8)) return false;
    int rows = (int)((budget - fixed) / (row + 8 + GJ_MB * 8));              // each row: z or panel column, 1/d, Cj
    if (rows > LZ_MAXR) rows = LZ_MAXR;
    int mb = rows / 3;
    if (mb > GJ_MB) mb = GJ_MB;
    if (ld > 512 && mb > LZ_MT) mb = LZ_MT;                                  // the 1024-thread plan compiles the 8-column panel only
    if (mb < 2) mb = 2;
    *mb_out = mb; *rows_out = rows;
    *shmem_out = ((size_t)(rows + 4) * ld + ld + rows + GJ_MB + (size_t)(rows + 4) * GJ_MB + 2 * GJ_MB * GJ_MB + 2 * GJ_MB + 18) * 8 + 3 * (size_t)ld + 16;
    return true;
}

}  // namespace partls
