// nm_rows.h — what the sampler's host code (nm_api.hip) sees of its kernels (nm_rows.hip): a row of the configuration table NM_CFG_ROWS
// as data and function pointers, and the launches of the four small kernels.  No device code and no Cfg: nm_api.hip compiles without
// nm_kernels.h.  The names are the library's own (hidden visibility, as g_create_error).
#pragma once
#include "nm_params.h"

#include <hip/hip_runtime.h>
#include <stddef.h>

namespace nm {

#define NM_INTERNAL __attribute__((visibility("hidden")))

// The kernels of one row (potential, size class, workgroups per replica).  Every launch takes the grid (nm_api.hip nm_grid) and runs the row's
// block size and dynamic LDS.  plain: the production form (nm_kernels.h nm_block_body PLAIN) where the row has one; whether a call may run it
// is the host's decision (plain_call).
struct Row {
    int nmax;                                      // atoms the row's arrays hold
    size_t nbr_g_elems, aux_doubles, xbuf_doubles; // per slot: list entries in HBM, the spill of a workgroup, one hand-over buffer
    hipError_t (*block)(unsigned int grid, hipStream_t s, const KParams &p, bool plain);
    hipError_t (*cycles)(unsigned int grid, hipStream_t s, const KParams &p, bool plain); // nm_cycles_kernel, recording where p.rec is set; null: not a FUSED row
    hipError_t (*probe)(unsigned int grid, hipStream_t s, const KParams &p);              // the residency census alone
    hipError_t (*request_lds)();                   // dynamic LDS above 64 KiB has to be requested per kernel
    int (*blocks_per_cu)();                        // workgroups of the block kernel one CU admits (LDS, registers); 0 on an error
};
NM_INTERNAL const Row *nm_row(int pot, int kind, int q); // null: the table has no such row

NM_INTERNAL hipError_t launch_order(hipStream_t s, int nslots, const unsigned long long *ticks, int *order);
NM_INTERNAL hipError_t launch_adapt(hipStream_t s, int nslots, const int *slot2buf, double *steps, double *count, float *ratio, const int *halt);
NM_INTERNAL hipError_t launch_exchange(hipStream_t s, int nrows, int nt, int row0, uint32_t seed, uint32_t step, int *slot2buf, const double *therm,
                                       const double *et, const double *pf, const double *tape, double *crit_out, int *nswaps, const int *halt);
NM_INTERNAL hipError_t launch_record(hipStream_t s, const RecArgs &a);

#ifdef NM_PROF
// diagnostic build only: the device globals of nm_kernels.h, read where they are defined.  which 0: nm_oob_count, 1: nm_list_miss, both zeroed behind the read
NM_INTERNAL hipError_t prof_take_count(int which, unsigned int *count);
NM_INTERNAL hipError_t prof_miss_info(double *info16);
#endif

} // namespace nm
