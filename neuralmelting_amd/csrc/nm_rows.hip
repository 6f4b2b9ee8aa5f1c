// nm_rows.hip — the sampler's kernels (nm_kernels.h) behind nm_rows.h: the Cfg typedefs, the configuration table NM_CFG_ROWS and the launchers
// of every row.  No context logic: the host code (nm_api.hip) decides what is launched, with which parameters and in which form.
// One object: the compiler's code for a kernel depends on what else its translation unit holds (profiles/r22_split_sampler.txt: every split
// of the table over several objects that was tried moved production kernels), so all 88 kernels stay together.
#include "../../include/nm.h" // (NM_STATS_COLS, NM_TRACE_COLS: nm_kernels.h)
#include "nm_rows.h"

#include "nm_kernels.h"

#include <type_traits>

namespace nm {
namespace {

// The small kernels run 512 threads, 8 waves: 256 VGPRs per lane, no spills (1024 threads cap at 128 and spilled ~200).
// cluster variants of the small kernel: Q workgroups per replica, threads-per-atom scaled so that all 512 threads work
// (a cluster stores the list rows of its own atoms only, and keeps the list twice: a rejected move goes back to the one it started from)
typedef Cfg<512, 4, 256, 192, unsigned char, true, true, 0, 128, true, true> CfgSmallQ2;
typedef Cfg<512, 8, 256, 192, unsigned char, true, true, 0, 64, true, true> CfgSmallQ4;
typedef Cfg<512, 16, 256, 256, unsigned char, true, true, 0, 32, true, true> CfgSmallQ8; // grids of <= 32 replicas
typedef Cfg<512, 2, 256, 192, unsigned char, true, true, 0, 256, true, true> CfgSmall;     // N <= 256: everything incl. the byte lists in LDS
// element Al: Sutton-Chen EAM, 4^3 cells only (BASELINE config 4); 200 neighbour slots (134 within rc+skin in the crystal)
typedef Cfg<512, 2, 256, 256, unsigned char, true, true, 1> CfgSmallSC;
typedef Cfg<512, 4, 256, 256, unsigned char, true, true, 1, 128, true, true> CfgSmallSCQ2; // (own rows, two lists)
typedef Cfg<512, 8, 256, 256, unsigned char, true, true, 1, 64, true, true> CfgSmallSCQ4;
// element Al at 5^3 to 8^3 cells: 16-bit lists in HBM/L2, chunked as CfgMid's and CfgLarge's, full lists (Cfg::HALF stays lj/cut's).  256 slots
// per atom: the crystal has 134 neighbours within rc + skin = 8.1 A, and the longest row over bench's Al grid (8 x 8, P 1 .. 8 bar, T 256 .. 2560 K,
// 40 cycles from the lattice) was 149 at 5^3 and 151 at 8^3; more is reported as ST_LIST_OVERFLOW.  Densities in LDS at 864 atoms (141.5 KB in all), in the spill at 2048
// (Cfg::RHO_LDS: positions, velocities and forces alone take 144 KB there).
typedef Cfg<512, 1, 864, 256, unsigned short, false, true, 1> CfgMidSC;     // 1 and 2 workgroups per replica
typedef Cfg<512, 2, 864, 256, unsigned short, false, true, 1> CfgMidSCQ4;   // 4
typedef Cfg<512, 1, 2048, 256, unsigned short, false, false, 1> CfgLargeSC; // 1, 2 and 4
// elements Cu and Ni: every Al configuration again with the Sutton-Chen exponent n = 9 (Cfg POT 2).  Their cutoff and skin are Al's in units of
// the lattice constant (nm_lattice.h sc_element), so the list lengths, the 256 slots, the LDS plans and the size thresholds above hold for them unchanged.
typedef Cfg<512, 2, 256, 256, unsigned char, true, true, 2> CfgSmallSC9;
typedef Cfg<512, 4, 256, 256, unsigned char, true, true, 2, 128, true, true> CfgSmallSC9Q2;
typedef Cfg<512, 8, 256, 256, unsigned char, true, true, 2, 64, true, true> CfgSmallSC9Q4;
typedef Cfg<512, 1, 864, 256, unsigned short, false, true, 2> CfgMidSC9;
typedef Cfg<512, 2, 864, 256, unsigned short, false, true, 2> CfgMidSC9Q4;
typedef Cfg<512, 1, 2048, 256, unsigned short, false, false, 2> CfgLargeSC9;
typedef Cfg<512, 1, 864, 192, unsigned short, false, true> CfgMid;     // N <= 864: list in HBM/L2, saved copies in LDS (here: at 2 workgroups per replica)
// the same at ONE workgroup per replica (more replicas than CUs: the reference's run.sh setting): every pair lies inside the workgroup and
// is listed once (Cfg::HALF, nm_kernels.h)
typedef Cfg<512, 1, 864, 192, unsigned short, false, true, 0, 864, true, false, true> CfgMidH;
// cluster variants: own atoms 216 / 108
typedef Cfg<512, 2, 864, 192, unsigned short, false, true> CfgMidQ4;
// 8 workgroups per replica: 108 own atoms, whose list rows (16-bit, 41 KB at 192 slots) fit in LDS once the saved velocities moved to the spill.
// 192 list slots per atom since round 4 (160 before): at the skin of 0.55 that these sizes now run with, the dense crystals of the P* = 7.5-8 rows
// reach 147 entries (scripts/probe_maxrow6.py)
typedef Cfg<512, 4, 864, 192, unsigned short, true, true, 0, 108, false> CfgMidQ8;
// N <= 2048: saved copies spill to HBM as well.  224 list slots: the list lives in HBM, so slots are cheap, and at skin 0.6 the dense
// crystals (P* = 8: 140 neighbours inside 3.1, the next shell of 36 just beyond) came within ~10 % of the 160 there were
typedef Cfg<512, 1, 2048, 224, unsigned short, false, false> CfgLarge;
// the same at ONE workgroup per replica (more replicas than CUs): half lists (Cfg::HALF), as CfgMidH.  Measured at 256 replicas of 2048 atoms: 254 k
// against 231 k sweeps/s sustained (+10 %)
typedef Cfg<512, 1, 2048, 224, unsigned short, false, false, 0, 2048, false, false, true> CfgLargeH;

// The configuration a context runs: X(pot, kind, Q, Cfg, FUSED) for the potential (nm_ctx::pot), the size class (nm_ctx::kind: the first
// kind whose NMAX holds N) and the workgroups per replica (nm_ctx::cus).  FUSED: nm_cycles_kernel is instantiated for the row (nm_api.hip
// cycles_kind_ok decides where it runs).  Block launches, the occupancy query, the residency probe, the fused launch and the buffer sizes all find
// their configuration here (with_row, handed to the host as nm_row's Row), and pick_q only picks a Q that has a row.  One row per line:
// tests/helpers.py reads the table.
#define NM_CFG_ROWS(X)                  \
    X(0, 0, 1, CfgSmall,          0)    \
    X(0, 0, 2, CfgSmallQ2,        1)    \
    X(0, 0, 4, CfgSmallQ4,        1)    \
    X(0, 0, 8, CfgSmallQ8,        1)    \
    X(0, 1, 1, CfgMidH,           0)    \
    X(0, 1, 2, CfgMid,            0)    \
    X(0, 1, 4, CfgMidQ4,          0)    \
    X(0, 1, 8, CfgMidQ8,          1)    \
    X(0, 2, 1, CfgLargeH,         0)    \
    X(0, 2, 2, CfgLarge,          0)    \
    X(0, 2, 4, CfgLarge,          0)    \
    X(1, 0, 1, CfgSmallSC,        0)    \
    X(1, 0, 2, CfgSmallSCQ2,      1)    \
    X(1, 0, 4, CfgSmallSCQ4,      1)    \
    X(1, 1, 1, CfgMidSC,          0)    \
    X(1, 1, 2, CfgMidSC,          0)    \
    X(1, 1, 4, CfgMidSCQ4,        0)    \
    X(1, 2, 1, CfgLargeSC,        0)    \
    X(1, 2, 2, CfgLargeSC,        0)    \
    X(1, 2, 4, CfgLargeSC,        0)    \
    X(2, 0, 1, CfgSmallSC9,       0)    \
    X(2, 0, 2, CfgSmallSC9Q2,     1)    \
    X(2, 0, 4, CfgSmallSC9Q4,     1)    \
    X(2, 1, 1, CfgMidSC9,         0)    \
    X(2, 1, 2, CfgMidSC9,         0)    \
    X(2, 1, 4, CfgMidSC9Q4,       0)    \
    X(2, 2, 1, CfgLargeSC9,       0)    \
    X(2, 2, 2, CfgLargeSC9,       0)    \
    X(2, 2, 4, CfgLargeSC9,       0)

// f(Cfg(), std::bool_constant<FUSED>()) for the row (pot, kind, q); `none` where the table has no such row
template <class R, class F>
R with_row(int pot, int kind, int q, R none, F &&f)
{
#define NM_ROW(P, K, Q, C, FUSED) if (pot == P && kind == K && q == Q) return f(C(), std::bool_constant<FUSED>());
    NM_CFG_ROWS(NM_ROW)
#undef NM_ROW
    return none;
}

// every row fits the CU's LDS and holds the atoms of its kind (nm_create picks the kind by the Q = 1 row's NMAX); a half list runs at one
// workgroup per replica only (pair_vec_half takes every listed atom for an own atom)
#define NM_ROW(P, K, Q, C, FUSED) static_assert(C::LDS_BYTES <= 160 * 1024 && C::NMAX == (K == 0 ? 256 : K == 1 ? 864 : 2048) && (!C::HALF || Q == 1), #C);
NM_CFG_ROWS(NM_ROW)
#undef NM_ROW
static_assert(CfgMidSC::RHO_LDS && CfgMidSCQ4::RHO_LDS && !CfgLargeSC::RHO_LDS, "densities: in LDS at 864 atoms, in the spill at 2048");
// a cluster row with own-row lists in LDS runs at NMAX / NLIST workgroups per replica and at no other number: its production form has that
// number and the own range at compile time (Replica::FIXQ), whatever KParams::cus says
#define NM_ROW(P, K, Q, C, FUSED) static_assert(!(C::LIST_LDS && C::NLIST < C::NMAX) || Q * C::NLIST == C::NMAX, #C);
NM_CFG_ROWS(NM_ROW)
#undef NM_ROW

// the stage of the random numbers drawn ahead (Cfg::STAGE: 6.5 KB) exists for the 4^3 rows and no others, and none of them shares its CU with it
// any more than without it: every row asks for more than half of the 160 KB (and fits them: above).  CfgSmallQ8 stays inside the 82 KB floor;
// CfgSmallQ4, which laid out 79.25 KB, now asks for 85.75 KB; the other rows were above the floor before.
// Headroom: CfgSmall, the one-workgroup row with both lists of all 256 rows, now takes 161536 of the CU's 163840 bytes — 2304 are left.
#define NM_ROW(P, K, Q, C, FUSED) static_assert(C::STAGE == (K == 0) && (K != 0 || 2 * C::LDS_BYTES > 160 * 1024), #C);
NM_CFG_ROWS(NM_ROW)
#undef NM_ROW

// The production form of the block (nm_block_body's PLAIN) is instantiated for the 4^3 rows, kind 0, whose NMAX the static_assert above
// ties to 256: block and fused kernels.  The 864- and 2048-atom rows keep the general form alone (build time).
template <class C> constexpr bool has_plain = C::NMAX == 256;

template <class C, bool PLAIN>
hipError_t launch_block_form(unsigned int grid, hipStream_t s, const KParams &p)
{
    hipLaunchKernelGGL((nm_block_kernel<C, PLAIN>), dim3(grid), dim3(C::BLOCK), C::LDS_BYTES, s, p);
    return hipGetLastError();
}

template <class C>
hipError_t launch_block(unsigned int grid, hipStream_t s, const KParams &p, bool plain)
{
    if constexpr (has_plain<C>)
        if (plain) return launch_block_form<C, true>(grid, s, p);
    return launch_block_form<C, false>(grid, s, p);
}

template <class C>
hipError_t launch_probe(unsigned int grid, hipStream_t s, const KParams &p)
{
    const hipError_t e = hipFuncSetAttribute((const void *)nm_probe_kernel<C>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)C::LDS_BYTES);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(nm_probe_kernel<C>, dim3(grid), dim3(C::BLOCK), C::LDS_BYTES, s, p);
    return hipGetLastError();
}

// dynamic LDS above 64 KiB has to be requested per kernel
template <class C>
hipError_t request_lds()
{
    if constexpr (has_plain<C>) {
        const hipError_t e = hipFuncSetAttribute((const void *)nm_block_kernel<C, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)C::LDS_BYTES);
        if (e != hipSuccess) return e;
    }
    return hipFuncSetAttribute((const void *)nm_block_kernel<C, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)C::LDS_BYTES);
}

// workgroups of the block kernel one CU admits (LDS, registers)
template <class C>
int blocks_per_cu()
{
    int n = 0;
    if (request_lds<C>() != hipSuccess) return 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, nm_block_kernel<C>, C::BLOCK, C::LDS_BYTES) != hipSuccess) return 0;
    return n;
}

template <class C, bool REC, bool PLAIN>
hipError_t launch_cycles_form(unsigned int grid, hipStream_t s, const KParams &p)
{
    const hipError_t e = hipFuncSetAttribute((const void *)nm_cycles_kernel<C, REC, PLAIN>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)C::LDS_BYTES);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((nm_cycles_kernel<C, REC, PLAIN>), dim3(grid), dim3(C::BLOCK), C::LDS_BYTES, s, p);
    return hipGetLastError();
}
template <class C, bool REC>
hipError_t launch_cycles_rec(unsigned int grid, hipStream_t s, const KParams &p, bool plain)
{
    if constexpr (has_plain<C>)
        if (plain) return launch_cycles_form<C, REC, true>(grid, s, p);
    return launch_cycles_form<C, REC, false>(grid, s, p);
}
// the recording instantiation where the launch has a ring (KParams::rec), the outputs-off one elsewhere: the same configurations have both
template <class C>
hipError_t launch_cycles(unsigned int grid, hipStream_t s, const KParams &p, bool plain)
{
    return p.rec ? launch_cycles_rec<C, true>(grid, s, p, plain) : launch_cycles_rec<C, false>(grid, s, p, plain);
}

// nm_cycles_kernel is instantiated for the FUSED rows alone (the 4^3 clusters and the 6^3 cluster of eight)
template <class C, bool FUSED>
constexpr decltype(Row::cycles) cycles_of()
{
    if constexpr (FUSED) return launch_cycles<C>;
    else return nullptr;
}

template <class C, bool FUSED>
const Row *row_of()
{
    static const Row r = { C::NMAX, C::NBR_G_ELEMS, C::AUX_DOUBLES, C::XBUF_DOUBLES, launch_block<C>, cycles_of<C, FUSED>(), launch_probe<C>, request_lds<C>, blocks_per_cu<C> };
    return &r;
}

} // namespace

const Row *nm_row(int pot, int kind, int q)
{
    return with_row(pot, kind, q, (const Row *)nullptr, [](auto cfg, auto fused) { return row_of<decltype(cfg), decltype(fused)::value>(); });
}

hipError_t launch_order(hipStream_t s, int nslots, const unsigned long long *ticks, int *order)
{
    hipLaunchKernelGGL(nm_order_kernel, dim3((nslots + 255) / 256), dim3(256), 0, s, nslots, ticks, order);
    return hipGetLastError();
}

hipError_t launch_adapt(hipStream_t s, int nslots, const int *slot2buf, double *steps, double *count, float *ratio, const int *halt)
{
    hipLaunchKernelGGL(nm_adapt_kernel, dim3((nslots + 63) / 64), dim3(64), 0, s, nslots, slot2buf, steps, count, ratio, halt);
    return hipGetLastError();
}

hipError_t launch_exchange(hipStream_t s, int nrows, int nt, int row0, uint32_t seed, uint32_t step, int *slot2buf, const double *therm,
                           const double *et, const double *pf, const double *tape, double *crit_out, int *nswaps, const int *halt)
{
    hipLaunchKernelGGL(nm_exchange_kernel, dim3(1), dim3(64), 0, s, nrows, nt, row0, seed, step, slot2buf, therm, et, pf, tape, crit_out, nswaps, halt);
    return hipGetLastError();
}

hipError_t launch_record(hipStream_t s, const RecArgs &a)
{
    hipLaunchKernelGGL(nm_record_kernel, dim3(a.nslots), dim3(256), 0, s, a);
    return hipGetLastError();
}

#ifdef NM_PROF
hipError_t prof_take_count(int which, unsigned int *count)
{
    const unsigned int zero = 0;
    hipError_t e = which == 0 ? hipMemcpyFromSymbol(count, HIP_SYMBOL(nm_oob_count), sizeof(unsigned int))
                              : hipMemcpyFromSymbol(count, HIP_SYMBOL(nm_list_miss), sizeof(unsigned int));
    if (e != hipSuccess) return e;
    return which == 0 ? hipMemcpyToSymbol(HIP_SYMBOL(nm_oob_count), &zero, sizeof(unsigned int))
                      : hipMemcpyToSymbol(HIP_SYMBOL(nm_list_miss), &zero, sizeof(unsigned int));
}
hipError_t prof_miss_info(double *info16) { return hipMemcpyFromSymbol(info16, HIP_SYMBOL(nm_miss_info), 16 * sizeof(double)); }
#endif

} // namespace nm
