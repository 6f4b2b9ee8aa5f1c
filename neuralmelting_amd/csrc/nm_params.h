// nm_params.h — the plain structs and constants that the sampler's host code (nm_api.hip) and its kernels (nm_device.h, nm_kernels.h)
// share: the kernels' arguments, the status bits and the layout of a recorded cycle.  No device code.
#pragma once
#include <stdint.h>

namespace nm {

// status bits per slot
enum : int { ST_LIST_OVERFLOW = 1, ST_BOX_TOO_SMALL = 2, ST_TAPE_EXHAUSTED = 4, ST_NONFINITE = 8, ST_SYNC_TIMEOUT = 16, ST_NOT_RESIDENT = 32,
             ST_FORCE_RANGE = 64 };

struct KParams {
    int N, nslots, slot0;          // atoms, local replicas, global index of local slot 0
    int mod, nstps, bulk, iter_revert;
    int eval_only;                 // nm_eval: evaluate the loaded states and leave
    int md_mode;                   // nm_run_md: velocities at T, then nstps velocity-Verlet steps, no Metropolis test
    uint32_t seed, step;
    double ppos, pvol, lat, mass;
    double kB, mvv2e, ftm2v, nktv2p;
    double rc, skin;
    double sc_eps, sc_a2, sc_c;    // Sutton-Chen EAM (element Al): E = eps [ 1/2 sum (a/r)^7 - c sum sqrt(rho) ], rho = sum (a/r)^6
    // per buffer
    double *x, *v, *box, *steps, *therm;
    // per slot
    double *count;
    float *ratio;
    const int *slot2buf;
    const double *et, *pf, *tq;
    int *status;
    double *stats;
    const double *tape;
    const int *tape_off;
    double *trace;                 // [slot][mod][4] or null
    double *evalU, *evalW, *evalF; // nm_eval outputs
    void *nbr_g;                   // global neighbour lists (N > 256): [slot][maxnb*N] uint16
    double *aux_g;                 // global spill of the saved copies (large N): [slot][AUX_DOUBLES(N)]
    unsigned long long *prof;      // diagnostic build only
    int cus;                       // workgroups (CUs) cooperating on one replica
    int dbg;                       // NM_DBG: timing experiments only (skips work, results are wrong)
    int inj_rebuild, inj_q;        // fault injection for the tests of the error path (NM_INJECT_OVERFLOW=n,q): the n-th list rebuild of
                                   // a block reports an overflow in workgroup q of every cluster; -1 = off
    unsigned long long *tline;     // experiment build only: 100 MHz timestamps of slot 0's evaluations [q][wave][eval][8]
    double *xbuf;                  // [slot][2][XBUF_DOUBLES]: force slices + partial sums exchanged inside a cluster
    uint32_t launch_id;            // distinguishes the granules of successive launches
    int plain_granules;            // 1: clusters found to sit on one XCD hand over through that XCD's L2 (plain stores); 0: always write-through
    unsigned int *census;          // cluster launches: arrival counter of the grid's workgroups, then one per cluster.  The counters only ever
                                   // grow: a launch is complete at census_base + its own count (no memset in front of every launch); the
                                   // host zeroes them, and the bases, after a census that was given up (abort bit) and before they could wrap
    unsigned int census_base, census_cbase; // what the grid's counter / every cluster's counter stood at before this launch
    int *status_acc;               // per slot: status bits of every block since the host last looked (status[] holds the last launch's)
    int *halt;                     // launch id of the first block that stopped on an error; later launches do nothing until the host
                                   // has dealt with it (nm_api.hip settle): a failed block never has successors running on its state
    const int *rerun_mask;         // re-issue of a block after a hand-over timeout: only the slots marked here run; null = all
    int inj_census;                // fault injection (NM_TESTING=1, NM_INJECT_CENSUS): this launch's residency census fails
    int over;                      // the grid holds more clusters than the chip at once: every cluster takes its own census (census[1 + cluster])
    const int *order;              // one workgroup per replica and more replicas than the chip holds at once: workgroup b runs slot order[b],
                                   // slowest first (by the time each slot's previous block took); null = identity
    unsigned long long *last_ticks; // per slot: duration of its last block (100 MHz ticks), what nm_order_kernel sorts by
    // nm_run_cycles (nm_cycles_kernel): several cycles of block / adapt / exchange in ONE launch; the replicas of a pressure row meet at the end of
    // every block, the rows never wait for one another
    int ncycles, nt, row0;         // cycles of this launch; temperatures per row; global index of the context's first row
    int draw_ahead;                // 1: the production form of the 4^3 kernels draws a move's random numbers under the exchange of the energy
                                   // evaluation in front of it; NM_DRAW_AHEAD=0: behind that exchange (A/B, tests).  (In the four bytes that
                                   // padded row0: no other member moves, and the kernels that do not read it stay what they were.)
    unsigned int *rowbar, *rowgo;  // per local row: workgroups arrived (monotonic within the launch), cycles released by the row's leader
    int *cyc_abort;                // set by whoever leaves the launch early: nobody waits for a row that will not complete
    int *nswaps;                   // accepted swaps of the launch (atomic)
    double *xcrit;                 // dh of every pair the exchange sweeps visit, [local row][pair] in sweep order (nm_get_exchange_crit)
    // nm_run_cycles_recorded (nm_cycles_kernel<C, true>): the record of cycle c of this launch for slot k is rec[(c nslots + k) (3N + NM_REC_HEAD)],
    // tagged rec_tag0 + c once the slot's block of that cycle has completed
    double *rec;
    uint32_t rec_tag0;
    int start_handover;            // NM_START_HANDOVER=1: every trajectory starts with the hand-over of the first step's positions (A/B, tests)
};

// one slot's record of a recorded cycle: the 17 thermo columns (remcmc:208), box, tag, then x[3N]
enum : int { NM_REC_HEAD = 19, NM_REC_BOX = 17, NM_REC_TAG = 18 };

// nm_record_kernel's arguments (nm_kernels.h)
struct RecArgs { const double *x, *box, *therm, *steps, *count; const float *ratio; const int *slot2buf, *halt; double *dst; int nslots, N; uint32_t tag; };

} // namespace nm
