// nm_api.hip — C-ABI (include/nm.h) over the gfx950 kernels.  The context owns all device and pinned memory, its two HIP
// streams and its HIP events through the types of nm_own.h, which release them; nothing here falls back to a CPU path: without a
// usable HIP device nm_create fails with NM_ERR_HIP.  Host code only: the kernels, their configuration table and their
// launchers are nm_rows.hip, reached through the rows of nm_rows.h.
#include "../../include/nm.h"
#include "nm_lattice.h"
#include "nm_own.h"
#include "nm_rows.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>
#include <string>
#include <vector>

using namespace nm;

// what nm_last_error(NULL) returns: the message of a call that failed without a context.  nm_io.cpp's nm_lattice_state has none
// either and writes it too, so it is the one name the two files share
namespace nm { __attribute__((visibility("hidden"))) thread_local std::string g_create_error; }

namespace {

struct EvPair { Event a, b; bool used = false; uint32_t launch_id = 0; };

} // namespace

struct nm_ctx {
    nm_config cfg;
    int N, nslots, slot0, kind; // kind: 0 small, 1 mid, 2 large
    int cus;                    // workgroups per replica
    const Row *row;             // the kernels of (pot, kind, cus), nm_rows.h; set with cus (set_q)
    bool whole_rows;            // the slot range is made of whole pressure rows (nm_exchange can run on the device)
    uint32_t launch_id;
    int start_handover = 0; // NM_START_HANDOVER=1 (read once, nm_create): the 4^3 cluster kernels start every trajectory with a hand-over
    int draw_ahead = 1;     // NM_DRAW_AHEAD=0 (read once, nm_create): the production form of the 4^3 kernels draws behind the energy exchange, not under it
    double lat, mass, kB, mvv2e, ftm2v, nktv2p, skin, rc;
    int pot; // 0 lj/cut, 1 Sutton-Chen EAM n = 7 (Al), 2 Sutton-Chen EAM n = 9 (Cu, Ni): the kernels' Cfg POT
    double sc_eps, sc_a2, sc_c; // Sutton-Chen constants of the element (nm_lattice.h sc_element); unused by lj/cut
    uint32_t step;
    // The streams stand in front of everything that work on them can touch: members go in reverse order, so every buffer and event below is
    // released before the streams are destroyed, and ~nm_ctx has waited for both streams before the first member goes.  side: the rings' copies
    Stream stream, side;
    // device
    DevBuf<double> d_x, d_v, d_box, d_steps, d_therm, d_count, d_et, d_pf, d_tq, d_stats, d_xbuf;
    DevBuf<float> d_ratio;
    DevBuf<int> d_slot2buf, d_status, d_status_acc, d_halt, d_rerun, d_nswaps, d_order;
    DevBuf<unsigned long long> d_last_ticks;
    bool use_order; // one workgroup per replica and more replicas than CUs: launch the slowest slots first (nm_order_kernel)
    DevBuf<unsigned int> d_census; // residency census of cluster launches (nm_kernels.h): the grid's counter, then one per cluster
    unsigned int census_base = 0, census_cbase = 0; // what those counters stand at (they only grow; reset_census zeroes both)
    DevBuf<unsigned int> d_rowsync; // nm_run_cycles: per local row an arrival counter and a release word, then the abort word (KParams::rowbar, rowgo, cyc_abort)
    bool over;              // the grid holds twice the clusters the chip does at once (pick_q)
    // Calls queued on the stream since the host last looked at the outcome (settle): if a block of them stopped because its
    // cluster grid was not resident or a hand-over timed out, nothing after it has run (KParams::halt) and the same calls are
    // issued again with fewer workgroups per replica.
    struct Op { int kind, arg, trace; uint32_t step, launch_id; int rec = -1, rec0 = 0; }; // rec, rec0: ring and first cycle it records into (-1: none)
    std::vector<Op> journal;
    int heals = 0;              // blocks re-issued at a lower Q so far
    int cluster_launches = 0;   // (NM_INJECT_CENSUS counts these)
    std::string note;           // what nm_create's residency probe and later re-issues had to give up (nm_create_note)
    DevBuf<double> d_tape, d_xtape, d_trace, d_xcrit, d_evalU, d_evalW, d_evalF, d_aux; // d_trace: grown on demand (issue_block)
    DevBuf<int> d_tape_off;
    DevBuf<unsigned short> d_nbr;
    DevBuf<unsigned long long> d_prof; // diagnostic build only (NM_PROF)
    DevBuf<unsigned long long> d_tline; // experiment build only
    // recorded cycles: rings 0 and 1 hold the records of nm_run_cycles_recorded calls, rings 2 and 3 those of nm_snapshot (one cycle each).  A ring
    // is a device buffer of cap cycles' records (nslots x (3N + NM_REC_HEAD) doubles per cycle) and its pinned host copy, which lands in one D2H on
    // the side stream (the main stream never waits for it) behind the ring's last record.  n: records of the call in it, next: the next one
    // nm_snapshot_fetch hands out (the ring is free when n == 0); tag0: the tag of its first record; dirty: settle re-issued launches that write it,
    // the host copy is stale
    struct Ring { DevBuf<double> d; PinBuf<double> h; Event taken, landed; int cap = 0, n = 0, next = 0; uint32_t tag0 = 0;
                  bool dirty = false; } ring[4];
    uint32_t rec_calls = 0;
    std::deque<int> fetchq; // the rings whose next records nm_snapshot_fetch hands out, oldest first
    // pinned host staging area, grown on demand: whole device arrays on their way between the caller's arrays and HBM (copy_staged), and the
    // volumes that go with a few boxes (copy_slots)
    PinBuf<double> h_stage;
    int trace_on, trace_mod;
    int xtape_n;
    std::vector<double> h_et, h_pf, h_tq;
    std::vector<float> h_P, h_T; // the context's own copy of the grids (cfg.P / cfg.T point here after nm_create)
    std::vector<EvPair> ev;
    int ev_next;
    int launches;
    double total_ms;
    std::string err;
    ~nm_ctx()
    {
        if (stream) hipStreamSynchronize(stream);
        if (side) hipStreamSynchronize(side);
    }
};

namespace {

int fail(nm_ctx *c, int code, const std::string &msg)
{
    if (c) c->err = msg; else g_create_error = msg;
    return code;
}

#define HIPCHK(c, call)                                                                              \
    do {                                                                                             \
        hipError_t e_ = (call);                                                                      \
        if (e_ != hipSuccess)                                                                        \
            return fail((c), NM_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_));         \
    } while (0)

// test-only environment hooks (NM_ASSUME_CUS, NM_INJECT_OVERFLOW, NM_INJECT_CENSUS) are honoured only under NM_TESTING=1, so that a
// stray variable cannot change Q or stop a production run
bool testing()
{
    const char *e = std::getenv("NM_TESTING");
    return e && std::atoi(e) != 0;
}

void fill_params(const nm_ctx *c, KParams &p)
{
    std::memset(&p, 0, sizeof p);
    p.N = c->N; p.nslots = c->nslots; p.slot0 = c->slot0;
    p.nstps = c->cfg.nstps; p.bulk = c->cfg.bulk; p.iter_revert = c->cfg.iter_revert;
    p.seed = c->cfg.seed; p.step = c->step;
    p.ppos = c->cfg.ppos; p.pvol = c->cfg.pvol; p.lat = c->lat; p.mass = c->mass;
    p.kB = c->kB; p.mvv2e = c->mvv2e; p.ftm2v = c->ftm2v; p.nktv2p = c->nktv2p;
    p.rc = c->rc; p.skin = c->skin;
    p.sc_eps = c->sc_eps; p.sc_a2 = c->sc_a2; p.sc_c = c->sc_c; // Sutton & Chen, Phil. Mag. Lett. 61 (1990) 139 (nm_lattice.h sc_element)
    p.x = c->d_x; p.v = c->d_v; p.box = c->d_box; p.steps = c->d_steps; p.therm = c->d_therm;
    p.count = c->d_count; p.ratio = c->d_ratio; p.slot2buf = c->d_slot2buf;
    p.et = c->d_et; p.pf = c->d_pf; p.tq = c->d_tq;
    p.status = c->d_status; p.stats = c->d_stats;
    p.tape = c->d_tape; p.tape_off = c->d_tape_off;
    p.nbr_g = c->d_nbr; p.aux_g = c->d_aux;
    p.prof = c->d_prof;
    p.cus = c->cus; p.xbuf = c->d_xbuf; p.launch_id = c->launch_id;
    p.census = c->cus > 1 ? c->d_census.p : nullptr; p.over = (c->cus > 1 && c->over) ? 1 : 0;
    p.census_base = c->census_base; p.census_cbase = c->census_cbase;
    p.plain_granules = 1;
    if (const char *e = std::getenv("NM_PLAIN_GRANULES")) p.plain_granules = std::atoi(e);
    p.start_handover = c->start_handover;
    p.draw_ahead = c->draw_ahead;
    p.dbg = 0;
    p.tline = c->d_tline;
    if (const char *e = std::getenv("NM_DBG")) p.dbg = std::atoi(e);
    p.inj_rebuild = -1; p.inj_q = 0;
    const char *e = testing() ? std::getenv("NM_INJECT_OVERFLOW") : nullptr; // tests of the error path only
    if (e) {
        int n = -1, q = 0;
        if (std::sscanf(e, "%d,%d", &n, &q) >= 1) { p.inj_rebuild = n; p.inj_q = q; }
    }
    p.status_acc = c->d_status_acc; p.halt = c->d_halt; p.rerun_mask = nullptr; p.inj_census = 0;
    p.order = (c->use_order && (c->cus == 1 || c->over)) ? c->d_order.p : nullptr; p.last_ticks = c->d_last_ticks;
}

// workgroups of a launch: 8 Q ceil(nslots / 8), the block kernel's cluster mapping (nm_kernels.h); nslots x Q when 8 divides nslots or Q = 1
unsigned int nm_grid(int nslots, int q) { return q == 1 ? (unsigned int)nslots : (unsigned int)(8 * q * ((nslots + 7) / 8)); }
size_t census_words(int nslots) { return 1 + (size_t)8 * ((nslots + 7) / 8); } // the grid's counter + one per cluster

// The production form of the block (nm_kernels.h nm_block_body's PLAIN; the rows that have one: nm_rows.hip) runs exactly where the call asks for
// nothing it leaves out: bulk position moves, no RNG tape, no trace, not nm_run_md, no forces out of nm_eval.  NM_PLAIN_KERNELS=0 forces the general
// form (tests, A/B); both forms compute the same bits.  Full cells only: the atom count of the production form is its row's NMAX at compile
// time (nm_kernels.h Replica::FIXN), so every other atom count of the size class (108, 32, the ragged sizes of the tests) takes the general form.
bool plain_call(const KParams &p, const Row *row)
{
    const char *e = std::getenv("NM_PLAIN_KERNELS");
    if (e && !std::strcmp(e, "0")) return false;
    return p.bulk && !p.tape && !p.trace && !p.md_mode && !p.evalF && p.N == row->nmax;
}

// The census counters only grow (KParams::census_base): zero them and the bases.  At creation, around the residency probes, after a
// census that was given up (its abort bit would fail every later launch) and long before they could wrap.
hipError_t reset_census(nm_ctx *c)
{
    c->census_base = c->census_cbase = 0;
    return hipMemsetAsync(c->d_census, 0, sizeof(unsigned int) * census_words(c->nslots), c->stream);
}

// the workgroups per replica and the row of the configuration table that goes with them (null: the table has none; every launch then fails)
void set_q(nm_ctx *c, int q, bool over)
{
    c->cus = q; c->over = over;
    c->row = nm_row(c->pot, c->kind, q);
}

// nm_cycles_kernel is instantiated for the FUSED rows (the 4^3 clusters and the 6^3 cluster of eight).  nm_run_cycles uses it where it measured faster
// than the loop of single launches: the 4^3 clusters of 2 and 4 workgroups (64-128 replicas: +2.4 to +2.9 % LJ, +0.5 % Al).  Clusters of 8 run 32 replicas
// or fewer, whose rows have little spread to hide, and there the block compiled inside the loop over cycles (~1 % slower) costs more than the rows gain
// (-0.8 % at 4^3, -2.9 % at 6^3): the loop of single launches, unless NM_FUSED_CYCLES=all.  NM_FUSED_CYCLES=0: never.  DESIGN.md §7.4 (6).
bool cycles_kind_ok(const nm_ctx *c)
{
    if (!c->row || !c->row->cycles) return false;
    const char *e = std::getenv("NM_FUSED_CYCLES");
    if (e && !std::strcmp(e, "all")) return true;
    if (e && !std::strcmp(e, "0")) return false;
    return c->kind == 0 && (c->cus == 2 || c->cus == 4);
}

hipError_t launch_cycles_kind(const nm_ctx *c, const KParams &p)
{
    if (!c->row || !c->row->cycles) return hipErrorInvalidDeviceFunction;
    return c->row->cycles(nm_grid(c->nslots, c->cus), c->stream, p, plain_call(p, c->row));
}

hipError_t launch_kind(const nm_ctx *c, const KParams &p)
{
    if (!c->row) return hipErrorInvalidDeviceFunction;
    if (p.order) { // longest first, by what each slot's previous block took
        const hipError_t e = launch_order(c->stream, c->nslots, c->d_last_ticks, c->d_order);
        if (e != hipSuccess) return e;
    }
    return c->row->block(nm_grid(c->nslots, c->cus), c->stream, p, plain_call(p, c->row));
}

// 0 where the table has no configuration at q: pick_q then finds no room for such a grid
int blocks_per_cu_kind(const nm_ctx *c, int q)
{
    const Row *r = nm_row(c->pot, c->kind, q);
    return r ? r->blocks_per_cu() : 0;
}

hipError_t probe_kind(const nm_ctx *c, KParams p)
{
    if (!c->row) return hipErrorInvalidDeviceFunction;
    const hipError_t e = hipMemsetAsync(c->d_census, 0, sizeof(unsigned int) * census_words(c->nslots), c->stream);
    if (e != hipSuccess) return e;
    p.census_base = p.census_cbase = 0; // (the probe starts from zeroed counters; pick_q zeroes them again behind it)
    return c->row->probe(nm_grid(c->nslots, c->cus), c->stream, p);
}

// drain one event pair into the timing accumulators
void harvest(nm_ctx *c, EvPair &e)
{
    if (!e.used) return;
    hipEventSynchronize(e.b);
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess) { c->total_ms += ms; c->launches += 1; }
    e.used = false;
}

std::string status_text(const nm_ctx *c, int k, int bits)
{
    char buf[768];
    std::snprintf(buf, sizeof buf,
                  "replica slot %d (global %d) left the supported regime:%s%s%s%s%s%s%s", k, c->slot0 + k,
                  (bits & ST_LIST_OVERFLOW) ? " neighbour list overflow;" : "",
                  (bits & ST_BOX_TOO_SMALL) ? " box edge < 2*rc (minimum image invalid);" : "",
                  (bits & ST_TAPE_EXHAUSTED) ? " rng tape exhausted;" : "",
                  (bits & ST_NONFINITE) ? " non-finite energy;" : "",
                  (bits & ST_SYNC_TIMEOUT) ? " cluster hand-off timed out (workgroups not co-resident?);" : "",
                  (bits & ST_NOT_RESIDENT) ? " the launch's workgroups were not resident together (CUs taken by another process, stream or a CU "
                                             "mask): nothing was changed;" : "",
                  (bits & ST_FORCE_RANGE) ? " force outside the fixed-point range of the half-list kernel (a pair closer than 0.604 sigma);" : "");
    return buf;
}

enum : int { OP_BLOCK = 0, OP_ADAPT = 1, OP_EXCHANGE = 2, OP_MD = 3, OP_CYCLES = 4, OP_RECORD = 5 }; // OP_CYCLES: arg = MOD, trace = number of cycles;
// OP_RECORD: the record of cycle rec0 into ring rec (nm_run_cycles_recorded on the loop of single launches)

// ---- the queued calls (nm_run_block, nm_run_md, nm_adapt, nm_exchange) as stream operations; issued by the API call and, after a
// block had to be given up, again by settle()
int check_status(nm_ctx *c);

// a cluster launch has been queued: where its census leaves the counters
void census_advance(nm_ctx *c)
{
    if (c->cus <= 1) return;
    if (c->over) c->census_cbase += (unsigned int)c->cus; else c->census_base += nm_grid(c->nslots, c->cus);
}
void fill_census(const nm_ctx *c, KParams &p) { p.census_base = c->census_base; p.census_cbase = c->census_cbase; }

// one launch of the block (launch_kind) or of the fused cycles (launch_cycles_kind); timed: between an event pair that nm_timing_get harvests
int issue_launch(nm_ctx *c, hipError_t (*launch)(const nm_ctx *, const KParams &), const KParams &p, bool timed, uint32_t id)
{
    if (!timed) { HIPCHK(c, launch(c, p)); return NM_OK; }
    EvPair &e = c->ev[c->ev_next];
    harvest(c, e);
    HIPCHK(c, hipEventRecord(e.a, c->stream));
    HIPCHK(c, launch(c, p));
    HIPCHK(c, hipEventRecord(e.b, c->stream));
    e.used = true; e.launch_id = id;
    c->ev_next = (c->ev_next + 1) % (int)c->ev.size();
    return NM_OK;
}

int issue_block(nm_ctx *c, int kind, int arg, uint32_t step, int trace, const int *d_mask, bool timed)
{
    if (c->journal.size() > 4096 && !d_mask) { // a caller that never looks: bound the journal
        const int rc = check_status(c);
        if (rc) return rc;
    }
    ++c->launch_id;
    KParams p;
    const uint32_t keep = c->step;
    c->step = step;
    fill_params(c, p);
    c->step = keep;
    p.rerun_mask = d_mask;
    if (kind == OP_MD) { p.mod = 1; p.md_mode = 1; p.nstps = arg; p.tape = nullptr; }
    else {
        p.mod = arg;
        if (trace) {
            const size_t need = (size_t)c->nslots * arg * NM_TRACE_COLS;
            HIPCHK(c, c->d_trace.reserve(need));
            if (!d_mask) HIPCHK(c, hipMemsetAsync(c->d_trace, 0, need * sizeof(double), c->stream));
            p.trace = c->d_trace;
            c->trace_mod = arg;
        }
    }
    if (testing())
        if (const char *e = std::getenv("NM_INJECT_CENSUS")) // "n": the context's n-th cluster launch fails its residency census
            if (c->cus > 1 && std::atoi(e) == c->cluster_launches) p.inj_census = 1;
    if (c->cus > 1) ++c->cluster_launches;
    // status[] holds the bits of the LAST launch (status_acc[] everything since the host last looked); a launch that finds the halt
    // word armed does nothing, and the memset in front of it must not wipe the failed block's bits: they are in status_acc[]
    // (status[]: cleared by each slot's writer inside the kernel; census counters: monotonic — no memsets in front of a launch)
    if (c->cus > 1 && (c->census_base > 0x3F000000u || c->census_cbase > 0x3F000000u)) { HIPCHK(c, reset_census(c)); fill_census(c, p); }
    if (const int rc = issue_launch(c, launch_kind, p, timed, c->launch_id)) return rc;
    census_advance(c);
    c->journal.push_back({ kind, arg, trace, step, c->launch_id });
    return NM_OK;
}

int issue_adapt(nm_ctx *c)
{
    HIPCHK(c, launch_adapt(c->stream, c->nslots, c->d_slot2buf, c->d_steps, c->d_count, c->d_ratio, c->d_halt));
    c->journal.push_back({ OP_ADAPT, 0, 0, 0u, 0u });
    return NM_OK;
}

int issue_exchange(nm_ctx *c, uint32_t step)
{
    HIPCHK(c, launch_exchange(c->stream, c->cfg.nrows, c->cfg.nt, c->cfg.row0, c->cfg.seed, step, c->d_slot2buf, c->d_therm, c->d_et, c->d_pf,
                              c->xtape_n ? c->d_xtape.p : nullptr, c->d_xcrit, c->d_nswaps, c->d_halt));
    c->journal.push_back({ OP_EXCHANGE, 0, 0, step, 0u });
    return NM_OK;
}

size_t rec_cycle_doubles(const nm_ctx *c) { return (size_t)c->nslots * ((size_t)3 * c->N + NM_REC_HEAD); } // one cycle's records

// the record of cycle j of ring r, copied on the stream behind that cycle's block (nm_snapshot, the loop of single launches)
int issue_record(nm_ctx *c, int r, int j)
{
    const nm_ctx::Ring &g = c->ring[r];
    RecArgs a;
    a.x = c->d_x; a.box = c->d_box; a.therm = c->d_therm; a.steps = c->d_steps; a.count = c->d_count; a.ratio = c->d_ratio; a.slot2buf = c->d_slot2buf;
    a.halt = c->d_halt; a.dst = g.d + (size_t)j * rec_cycle_doubles(c); a.nslots = c->nslots; a.N = c->N; a.tag = g.tag0 + (uint32_t)j;
    HIPCHK(c, launch_record(c->stream, a));
    nm_ctx::Op o{ OP_RECORD, 0, 0, 0u, 0u };
    o.rec = r; o.rec0 = j;
    c->journal.push_back(o);
    return NM_OK;
}

// nm_run_cycles as stream operations: ONE launch of nm_cycles_kernel where the configuration has one and the whole grid is resident and checked by the
// census (clusters), else the same cycles as single blocks, adapts and exchanges.  rec >= 0 (nm_run_cycles_recorded): cycle k's record goes to cycle
// rec0 + k of ring rec — written by the fused kernel itself, or copied behind each block of the loop
int issue_cycles(nm_ctx *c, int ncycles, int mod, uint32_t step, bool timed, int rec, int rec0)
{
    const bool fused = c->whole_rows && c->cus > 1 && !c->over && cycles_kind_ok(c) && !c->d_tape && !c->xtape_n && !c->trace_on &&
                       !(c->use_order && (c->cus == 1 || c->over));
    if (!fused) {
        for (int k = 0; k < ncycles; ++k) {
            int rc = issue_block(c, OP_BLOCK, mod, step + (uint32_t)k, 0, nullptr, timed);
            if (!rc && rec >= 0) rc = issue_record(c, rec, rec0 + k);
            if (!rc) rc = issue_adapt(c);
            if (!rc) rc = issue_exchange(c, step + (uint32_t)k);
            if (rc) return rc;
        }
        return NM_OK;
    }
    // a launch holds at most 64 cycles (what the rows gain by not waiting is there after ~10; a kernel that runs for minutes serves nobody)
    constexpr int MAX_PER_LAUNCH = 64;
    if (ncycles > MAX_PER_LAUNCH) {
        for (int k = 0; k < ncycles; k += MAX_PER_LAUNCH) {
            const int rc = issue_cycles(c, std::min(MAX_PER_LAUNCH, ncycles - k), mod, step + (uint32_t)k, timed, rec, rec >= 0 ? rec0 + k : 0);
            if (rc) return rc;
        }
        return NM_OK;
    }
    const int nrows = c->cfg.nrows;
    if (!c->d_rowsync) HIPCHK(c, c->d_rowsync.alloc((size_t)2 * nrows + 2));
    HIPCHK(c, hipMemsetAsync(c->d_rowsync, 0, sizeof(unsigned int) * ((size_t)2 * nrows + 2), c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_nswaps, 0, sizeof(int), c->stream));
    const uint32_t first_id = c->launch_id + 1;
    c->launch_id += (uint32_t)ncycles;   // one id per cycle: the hand-over granules of successive blocks must differ
    KParams p;
    const uint32_t keep = c->step;
    c->step = step;
    fill_params(c, p);
    c->step = keep;
    p.launch_id = first_id;
    p.mod = mod; p.ncycles = ncycles; p.nt = c->cfg.nt; p.row0 = c->cfg.row0;
    p.rowbar = c->d_rowsync; p.rowgo = c->d_rowsync + nrows; p.cyc_abort = (int *)(c->d_rowsync + 2 * nrows); p.nswaps = c->d_nswaps; p.xcrit = c->d_xcrit;
    p.order = nullptr; p.tape = nullptr; p.trace = nullptr;
    if (rec >= 0) { p.rec = c->ring[rec].d + (size_t)rec0 * rec_cycle_doubles(c); p.rec_tag0 = c->ring[rec].tag0 + (uint32_t)rec0; }
    if (testing())
        if (const char *e = std::getenv("NM_INJECT_CENSUS"))
            if (std::atoi(e) == c->cluster_launches) p.inj_census = 1;
    ++c->cluster_launches;
    if (c->census_base > 0x3F000000u || c->census_cbase > 0x3F000000u) { HIPCHK(c, reset_census(c)); fill_census(c, p); }
    if (const int rc = issue_launch(c, launch_cycles_kind, p, timed, first_id)) return rc;
    census_advance(c);
    nm_ctx::Op o{ OP_CYCLES, mod, ncycles, step, first_id };
    o.rec = rec; o.rec0 = rec0; // (a re-issue records into the same ring)
    c->journal.push_back(o);
    return NM_OK;
}

// Workgroups per replica.  A cluster spins on its peers, so every workgroup of the grid must be resident at once.  The candidates
// are the Q <= qmax with a row in NM_CFG_ROWS for which the occupancy query admits the whole grid (workgroups per CU x CUs); the first one whose grid
// actually gathers in a residency census (nm_probe_kernel: the block kernel's launch shape, census only, nm_kernels.h) is taken,
// so a masked or busy CU lowers Q instead of stalling every block.  Leaves c->cus set; 1 when no cluster gathers.
int pick_q(nm_ctx *c, int qmax, std::string &note)
{
    hipDeviceProp_t prop;
    HIPCHK(c, hipGetDeviceProperties(&prop, c->cfg.device));
    int cu = prop.multiProcessorCount;
    if (testing())
        if (const char *e = std::getenv("NM_ASSUME_CUS")) { const int v = std::atoi(e); if (v > 0) cu = v; } // tests of the fallback
    set_q(c, 1, false);
    // The large cells (N > 864) at 4 workgroups per replica when that makes a grid of (nearly) TWICE the chip: the clusters run in
    // two rounds, longest block first, each with its own census.  Their blocks differ by more than 2x across an equilibrated PxT grid
    // (31-73 ms at 8^3, two workgroups each), so a resident grid of two workgroups per replica lasts as long as its slowest member while
    // a third of the CUs have nothing left to do; four workgroups make a block ~1.6x shorter, and two rounds of them, dealt out longest first,
    // end within a few ms of one another.  Measured on C5's per-GPU share (128 x 2048 atoms): equilibrated chains 221 k sweeps/s against
    // 211 k for the resident grid (+4.5 %: 74 ms per launch where perfect packing of the same blocks would give 67), but 276 k against
    // 324 k while all replicas are still alike (nothing to even out, and 4 workgroups per replica cost 1.27x the CU time of 2).  So it
    // is opt-in: NM_OVERSUBSCRIBE=1 (and a hundred cycles on, 203 k against 219 k: the gain belongs to the cycles in which the replicas differ most).  (It also leans on workgroups being dispatched in index order within an XCD, which HIP does not
    // promise; a cluster whose members do not gather fails its census and the block is re-issued on the resident grid, settle().)
    bool try_over = false;
    if (const char *e = std::getenv("NM_OVERSUBSCRIBE")) try_over = c->kind == 2 && qmax >= 4 && std::atoi(e) != 0;
    for (int pass = try_over ? 0 : 1; pass < 2; ++pass)
    for (int qq : { 8, 4, 2 }) {
        if (qq > qmax) continue;
        const int per_cu = blocks_per_cu_kind(c, qq); // (0 where the table has no configuration at qq)
        const long grid = (long)nm_grid(c->nslots, qq), room = (long)per_cu * cu;
        const bool over = pass == 0;
        if (over) { if (qq != 4 || grid > 2 * room || 4 * grid < 7 * room) continue; } // 1.75 .. 2 chips' worth of workgroups
        else if (grid > room) continue;
        set_q(c, qq, over); // probe: does the grid of this Q gather?
        KParams p;
        fill_params(c, p);
        p.status_acc = nullptr; p.halt = nullptr;
        HIPCHK(c, hipMemsetAsync(c->d_status, 0, sizeof(int) * c->nslots, c->stream));
        HIPCHK(c, probe_kind(c, p));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        std::vector<int> st((size_t)c->nslots);
        HIPCHK(c, hipMemcpy(st.data(), c->d_status, sizeof(int) * c->nslots, hipMemcpyDeviceToHost));
        bool ok = true;
        for (int v : st) ok = ok && !(v & ST_NOT_RESIDENT);
        HIPCHK(c, hipMemset(c->d_status, 0, sizeof(int) * c->nslots));
        HIPCHK(c, reset_census(c)); // (the probe's arrivals, or its abort bit, must not meet the first block)
        if (ok) return NM_OK;
        char buf[200];
        std::snprintf(buf, sizeof buf, "%d workgroups per replica (%d in all) did not gather on this device; falling back. ", qq, (int)nm_grid(c->nslots, qq));
        note += buf;
        set_q(c, 1, false);
    }
    return NM_OK;
}

// the buffers whose size depends on the workgroups per replica: the per-workgroup spill and the hand-over granules
int alloc_cluster_buffers(nm_ctx *c)
{
    const size_t ns = c->nslots;
    const size_t aux_doubles = c->row ? c->row->aux_doubles : 0, xbd = c->row ? c->row->xbuf_doubles : 0;
    // the new buffers first, swapped in only when both exist: a failure leaves the context with the buffers (and the workgroups per
    // replica) it can still run with
    DevBuf<double> aux, xbuf;
    hipError_t e = hipSuccess;
    if (aux_doubles) e = aux.alloc(ns * c->cus * aux_doubles);
    if (e == hipSuccess && c->cus > 1) e = xbuf.alloc_zeroed(ns * 2 * xbd);
    if (e != hipSuccess) {
        if (!c->d_xbuf) set_q(c, 1, false); // nothing to hand over with: one workgroup per replica (its spill area, if any, is a subset of what is there)
        return fail(c, NM_ERR_HIP, std::string("alloc_cluster_buffers: ") + hipGetErrorString(e));
    }
    c->d_aux = std::move(aux); c->d_xbuf = std::move(xbuf); // (empty where the row needs none: what was held is released either way)
    return NM_OK;
}

// The outcome of everything queued so far; the stream has been synchronised by the caller.  A block that stopped because its
// cluster grid was not resident (NM_ST_NOT_RESIDENT: nothing was touched) or a hand-over timed out (NM_ST_SYNC_TIMEOUT: the
// replicas concerned are as they were at the block's start) armed the halt word, so nothing queued behind it has run either
// (the reference's analogue is Dask retrying a failed gen_sample task, remcmc:921-922): the context drops to the next lower
// number of workgroups per replica that gathers and issues the same calls again — the failed block for the replicas that did
// not complete it, everything behind it as it was.  Any other status is the caller's to deal with: NM_ERR_STATE once, with
// the reason; the replicas' state is that of the failed block's start and the context stays usable.
int settle(nm_ctx *c)
{
    for (int round = 0; round < 4; ++round) {
        int halt = 0;
        HIPCHK(c, hipMemcpy(&halt, c->d_halt, sizeof(int), hipMemcpyDeviceToHost));
        std::vector<int> st((size_t)c->nslots);
        HIPCHK(c, hipMemcpy(st.data(), c->d_status_acc, sizeof(int) * c->nslots, hipMemcpyDeviceToHost));
        int any = 0;
        for (int v : st) any |= v;
        if (!halt && !any) { c->journal.clear(); c->err.clear(); return NM_OK; } // (nm_last_error is empty after a call that returned NM_OK)
        const int healable = ST_NOT_RESIDENT | ST_SYNC_TIMEOUT;
        size_t at = c->journal.size();
        bool mid_cycles = false; // the halt lies inside a launch of several cycles, behind its first: rows are at different cycles, nothing to re-issue
        for (size_t k = 0; k < c->journal.size(); ++k) {
            const nm_ctx::Op &o = c->journal[k];
            if ((o.kind == OP_BLOCK || o.kind == OP_MD) && (int)o.launch_id == halt) { at = k; break; }
            if (o.kind == OP_CYCLES && (uint32_t)halt >= o.launch_id && (uint32_t)halt < o.launch_id + (uint32_t)o.trace) {
                at = k; mid_cycles = (uint32_t)halt != o.launch_id || (any & ST_SYNC_TIMEOUT); break;
            }
        }
        if (halt && !(any & ~healable) && c->cus > 1 && at < c->journal.size() && !mid_cycles) {
            // ---- re-issue at a lower Q
            const int q_old = c->cus;
            std::string why;
            int rc = pick_q(c, q_old / 2, why);
            if (rc) return rc;
            HIPCHK(c, reset_census(c)); // (the failed launch's census may have left its abort bit)
            if ((rc = alloc_cluster_buffers(c))) return rc;
            std::vector<int> mask((size_t)c->nslots);
            for (int k = 0; k < c->nslots; ++k) mask[k] = st[k] ? 1 : 0;
            HIPCHK(c, hipMemcpy(c->d_rerun, mask.data(), sizeof(int) * c->nslots, hipMemcpyHostToDevice));
            HIPCHK(c, hipMemset(c->d_status_acc, 0, sizeof(int) * c->nslots));
            HIPCHK(c, hipMemset(c->d_halt, 0, sizeof(int)));
            char buf[256];
            std::snprintf(buf, sizeof buf, "block of step %u stopped at %d workgroups per replica (%s); re-issued at %d. %s",
                          c->journal[at].step, q_old, (any & ST_NOT_RESIDENT) ? "grid not resident" : "hand-over timed out", c->cus, why.c_str());
            c->note += buf;
            ++c->heals;
            // timing: the launch that halted did nothing for the replicas that are re-issued, and the blocks queued behind it found the
            // halt word armed and left at once — their event pairs would count launches that did no work.  Drop them (first wait for them:
            // an event pair is recycled) and time the re-issued blocks instead, so that nm_timing_get keeps meaning "the launches that did
            // the work".  nm_heal_count tells a caller that a region contained a re-issue.
            for (auto &e : c->ev)
                if (e.used && e.launch_id >= c->journal[at].launch_id) { hipEventSynchronize(e.b); e.used = false; }
            std::vector<nm_ctx::Op> todo(c->journal.begin() + at, c->journal.end());
            c->journal.clear();
            // records re-taken into a ring: its host copy (whose D2H must not overlap the re-issue) is stale, nm_snapshot_fetch copies again
            if (c->side) HIPCHK(c, hipStreamSynchronize(c->side));
            for (const nm_ctx::Op &o : todo)
                if (o.rec >= 0) c->ring[o.rec].dirty = true;
            for (size_t k = 0; k < todo.size(); ++k) {
                const nm_ctx::Op &o = todo[k];
                if (o.kind == OP_BLOCK || o.kind == OP_MD) rc = issue_block(c, o.kind, o.arg, o.step, o.trace, k == 0 ? c->d_rerun : nullptr, o.kind == OP_BLOCK);
                else if (o.kind == OP_CYCLES) rc = issue_cycles(c, o.trace, o.arg, o.step, true, o.rec, o.rec0); // (its census failed: nothing had run)
                else if (o.kind == OP_RECORD) rc = issue_record(c, o.rec, o.rec0);
                else if (o.kind == OP_ADAPT) rc = issue_adapt(c);
                else rc = issue_exchange(c, o.step);
                if (rc) return rc;
            }
            HIPCHK(c, hipStreamSynchronize(c->stream));
            continue; // look at the outcome of the re-issue
        }
        // ---- not curable here: report once, leave the context usable
        c->journal.clear();
        // launches queued behind the one that stopped found the halt word armed and left BEFORE their residency census, while the host had already
        // advanced the census base for them: start the counters afresh, or the next launch's census comes up short and is taken for a grid that
        // is not resident (re-issued at fewer workgroups per replica for no reason)
        if (halt) HIPCHK(c, reset_census(c));
        HIPCHK(c, hipMemcpy(c->d_status, st.data(), sizeof(int) * c->nslots, hipMemcpyHostToDevice)); // nm_get_status: what stopped which slot
        HIPCHK(c, hipMemset(c->d_status_acc, 0, sizeof(int) * c->nslots));
        HIPCHK(c, hipMemset(c->d_halt, 0, sizeof(int)));
        for (int k = 0; k < c->nslots; ++k)
            if (st[k]) return fail(c, NM_ERR_STATE, status_text(c, k, st[k]));
        return fail(c, NM_ERR_STATE, "a block stopped on an error that left no status bits");
    }
    return fail(c, NM_ERR_STATE, "a block could not be completed at any number of workgroups per replica");
}

int check_status(nm_ctx *c)
{
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return settle(c);
}

// the context's device, then the outcome of everything queued: a halted queue is re-issued, or its error reported, before anything
// it touches is read or replaced.  The opening of every entry point that does either, behind its argument checks
int settled(nm_ctx *c)
{
    HIPCHK(c, hipSetDevice(c->cfg.device));
    return check_status(c);
}

// slot -> buffer, as everything queued has left it (settled: it has run, or has been re-issued, before state is read or replaced)
int slot_map(nm_ctx *c, std::vector<int> &m)
{
    if (const int rc = settled(c)) return rc;
    m.resize(c->nslots);
    HIPCHK(c, hipMemcpy(m.data(), c->d_slot2buf, sizeof(int) * c->nslots, hipMemcpyDeviceToHost));
    return NM_OK;
}

// ---- state in and out.  Both directions, a range or a list of slots, any subset of the arrays (a null one is skipped) go through two routines:
// copy_slots, one small copy per slot and array, for a few slots, and copy_staged, whole device arrays through the pinned staging area, for
// many.  put: from the caller's arrays to the device (they are not written then); x, v [..][3N], box [..], dxdvdt [..][3], th [..][5] = temp,
// pe, ke, virial, vol (nm_set_thermo's columns), row q belonging to slot slot_of(q).  A box that is put takes its volume along (therm column 4).
hipError_t copy_row(nm_ctx *c, bool put, double *host, double *dev, size_t n)
{
    return put ? hipMemcpyAsync(dev, host, n * sizeof(double), hipMemcpyHostToDevice, c->stream)
               : hipMemcpyAsync(host, dev, n * sizeof(double), hipMemcpyDeviceToHost, c->stream);
}

// The listed buffers copied back to back on the context's stream, ONE wait (the split-row exchange re-seats the replicas that swapped,
// neuralmelting_amd/exchange.py).  The volumes go through the pinned staging area, so that nothing on this stack frame is read after return;
// a thermo row that is put lands behind its slot's box and volume
template <class SlotOf>
int copy_slots(nm_ctx *c, const std::vector<int> &m, bool put, int nk, SlotOf slot_of, double *x, double *v, double *box, double *dxdvdt, double *th)
{
    const size_t n3 = (size_t)3 * c->N;
    if (put) HIPCHK(c, c->h_stage.reserve((size_t)nk + 1));
    double *vol = c->h_stage;
    for (int q = 0; q < nk; ++q) {
        const size_t bq = (size_t)m[slot_of(q)];
        if (x) HIPCHK(c, copy_row(c, put, x + q * n3, c->d_x + bq * n3, n3));
        if (v) HIPCHK(c, copy_row(c, put, v + q * n3, c->d_v + bq * n3, n3));
        if (box) HIPCHK(c, copy_row(c, put, box + q, c->d_box + bq, 1));
        if (box && put) {
            vol[q] = std::pow(box[q], 3.0);
            HIPCHK(c, copy_row(c, put, vol + q, c->d_therm + 5 * bq + 4, 1));
        }
        if (dxdvdt) HIPCHK(c, copy_row(c, put, dxdvdt + 3 * q, c->d_steps + 3 * bq, 3));
        if (th) HIPCHK(c, copy_row(c, put, th + 5 * q, c->d_therm + 5 * bq, 5));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream)); // the caller's arrays (pageable: staged by the runtime) and the staging area are free again
    return NM_OK;
}

// Slots k0 .. k0 + nk - 1 through whole device arrays: one asynchronous copy per array and direction and one wait each way, instead of up
// to four small copies per replica.  A get reads the arrays back and gathers; a put scatters into the staging area, which a partial range
// first fills from the device (the merge; set-up path, not timed), and writes the arrays
int copy_staged(nm_ctx *c, const std::vector<int> &m, bool put, int k0, int nk, double *x, double *v, double *box, double *dxdvdt)
{
    const size_t n3 = (size_t)3 * c->N, ns = (size_t)c->nslots;
    HIPCHK(c, c->h_stage.reserve(2 * ns * n3 + 9 * ns));
    double *const hx = c->h_stage, *const ht = hx + 2 * ns * n3 + 4 * ns; // (therm: read and written with a box that is put, for its column 4)
    struct { double *host, *stage, *dev; size_t w; } const arr[] = { { x, hx, c->d_x, n3 }, { v, hx + ns * n3, c->d_v, n3 },
        { box, hx + 2 * ns * n3, c->d_box, 1 }, { dxdvdt, hx + 2 * ns * n3 + ns, c->d_steps, 3 } };
    const bool read_back = !put || nk != c->nslots;
    for (const auto &a : arr)
        if (a.host && read_back) HIPCHK(c, copy_row(c, false, a.stage, a.dev, ns * a.w));
    if (put && box) HIPCHK(c, copy_row(c, false, ht, c->d_therm, 5 * ns));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int q = 0; q < nk; ++q) {
        const size_t bq = (size_t)m[k0 + q];
        for (const auto &a : arr)
            if (a.host) {
                double *const h = a.host + q * a.w, *const s = a.stage + bq * a.w;
                std::memcpy(put ? s : h, put ? h : s, a.w * sizeof(double));
            }
        if (put && box) ht[5 * bq + 4] = std::pow(box[q], 3.0);
    }
    if (!put) return NM_OK;
    for (const auto &a : arr)
        if (a.host) HIPCHK(c, copy_row(c, true, a.stage, a.dev, ns * a.w));
    if (box) HIPCHK(c, copy_row(c, true, ht, c->d_therm, 5 * ns));
    HIPCHK(c, hipStreamSynchronize(c->stream)); // the staging area is reused by the next call
    return NM_OK;
}

// a range of slots: the few-slots path for at most 8 of them that are not all (the split-row exchange), else the staged arrays
int copy_range(nm_ctx *c, bool put, int k0, int nk, double *x, double *v, double *box, double *dxdvdt)
{
    std::vector<int> m;
    if (const int rc = slot_map(c, m)) return rc;
    if (nk <= 8 && nk < c->nslots) return copy_slots(c, m, put, nk, [k0](int q) { return k0 + q; }, x, v, box, dxdvdt, nullptr);
    return copy_staged(c, m, put, k0, nk, x, v, box, dxdvdt);
}

int copy_list(nm_ctx *c, const char *fn, bool put, int nk, const int *slots, double *x, double *v, double *box, double *dxdvdt, double *th)
{
    if (!c || nk < 0 || (nk && !slots)) return fail(c, NM_ERR_ARG, std::string(fn) + ": bad argument");
    for (int q = 0; q < nk; ++q)
        if (slots[q] < 0 || slots[q] >= c->nslots) return fail(c, NM_ERR_ARG, std::string(fn) + ": slot out of range");
    std::vector<int> m;
    if (const int rc = slot_map(c, m)) return rc;
    return copy_slots(c, m, put, nk, [slots](int q) { return slots[q]; }, x, v, box, dxdvdt, th);
}

} // namespace

extern "C" {

const char *nm_last_error(const nm_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }
const char *nm_create_note(const nm_ctx *ctx) { return ctx ? ctx->note.c_str() : ""; }
int nm_nslots(const nm_ctx *ctx) { return ctx ? ctx->nslots : NM_ERR_ARG; }
int nm_natoms(const nm_ctx *ctx) { return ctx ? ctx->N : NM_ERR_ARG; }
int nm_cus_per_replica(const nm_ctx *ctx) { return ctx ? ctx->cus : NM_ERR_ARG; }
int nm_heal_count(const nm_ctx *ctx) { return ctx ? ctx->heals : NM_ERR_ARG; }

// everything of nm_create behind its argument checks; a failure leaves its message in c->err and what was built so far to ~nm_ctx
static int init_ctx(nm_ctx *c, const nm_config *cfg)
{
    const bool by_slots = cfg->nslots > 0;
    c->cfg = *cfg;
    c->h_P.assign(cfg->P, cfg->P + cfg->np); c->h_T.assign(cfg->T, cfg->T + cfg->nt);
    c->cfg.P = c->h_P.data(); c->cfg.T = c->h_T.data();
    c->N = cfg->natoms;
    c->nslots = by_slots ? cfg->nslots : cfg->nrows * cfg->nt;
    c->slot0 = by_slots ? cfg->slot0 : cfg->row0 * cfg->nt;
    c->whole_rows = (c->slot0 % cfg->nt == 0) && (c->nslots % cfg->nt == 0);
    c->cfg.row0 = c->slot0 / cfg->nt;                       // meaningful only for whole rows
    c->cfg.nrows = c->whole_rows ? c->nslots / cfg->nt : 0;
    // (step, launch_id, the trace and tape settings, the timing accumulators: zero from `new nm_ctx()`)
    // material tables, remcmc:873-893
    // Verlet-list skin: not observable in results, only in the rebuild rate.  (Round 1 took 0.3, LAMMPS's lj default, as best at 256 atoms —
    // measured in the first cycles after the lattice start, when HMC steps are still short and rebuilds rare;
    // the O(N^2) rebuild of the larger cells favours fewer rebuilds (0.45: 6^3 -10 %, 8^3 -45 % per move)
    // (8^3, equilibrated chains, where a rebuild costs ~10 evaluations: 0.6 gives 107 ms per launch of C5's share against 121 at 0.45,
    // for +7 % while the chains still reject everything; 0.75 overflows the 160 list slots of the dense crystals)
    c->skin = cfg->natoms <= 512 ? 0.4 : cfg->natoms <= 1024 ? 0.55 : 0.6; // (256 atoms, equilibrated: 7.1 / 6.8 / 6.8 ms per launch at 0.3 / 0.4 / 0.5)
    // (round 4, sustained, same box each: 500 atoms at one workgroup per replica 1.385 / 1.411 / 1.392 / 1.390 M sweeps/s at 0.35 / 0.40 / 0.45 / 0.50;
    //  864 atoms: C3 share (Q = 8) 352 / 359 / 368 / 372 / 370 k at 0.40 / 0.45 / 0.50 / 0.55 / 0.60, 256 replicas at Q = 1 615 / 617 / 632 / 642 k at
    //  0.40 / 0.45 / 0.50 / 0.55: the O(N^2) rebuild of the larger cells wants fewer rebuilds; 0.45 for both until then)
    if (const char *e = std::getenv("NM_START_HANDOVER")) c->start_handover = std::atoi(e) != 0;
    if (const char *e = std::getenv("NM_DRAW_AHEAD")) c->draw_ahead = std::atoi(e) != 0;
    if (const char *e = std::getenv("NM_SKIN")) { const double v = std::atof(e); if (v > 0.0 && v < 1.0) c->skin = v; }
    c->lat = 1.122; c->mass = 1.0; c->kB = 1.0; c->mvv2e = 1.0; c->ftm2v = 1.0; c->nktv2p = 1.0;
    c->rc = 2.5; c->pot = 0; c->sc_eps = 0.0; c->sc_a2 = 0.0; c->sc_c = 0.0;
    if (const lat::ScElement *s = lat::sc_element(cfg->element)) { // units metal (LAMMPS update.cpp constants), remcmc:880-889
        c->lat = s->lat; c->mass = s->mass; c->kB = 8.617343e-5; c->mvv2e = 1.0364269e-4; c->ftm2v = 1.0 / 1.0364269e-4;
        c->nktv2p = 1.6021765e6; c->rc = s->rc; c->skin = s->skin; c->pot = s->pot; // (Al's skin: 0.8 until the rebuild's scan and append got cheaper
        // in round 3; equilibrated C4 on one box: 685 / 690 / 706 k sweeps/s at 0.8 / 0.7 / 0.6 A, 2.64 / 2.73 / 2.95 rebuilds per sweep)
        c->sc_eps = s->eps; c->sc_a2 = s->a * s->a; c->sc_c = s->c;
        if (cfg->element == NM_EL_AL) // (Al only)
            if (const char *e = std::getenv("NM_SKIN_AL")) { const double v = std::atof(e); if (v > 0.0 && v < 3.0) c->skin = v; }
    }

    // init_constant (remcmc:114-132) in float64 on the float32-rounded grid values (NumPy-1.x promotion)
    c->h_et.resize(c->nslots); c->h_pf.resize(c->nslots); c->h_tq.resize(c->nslots);
    for (int k = 0; k < c->nslots; ++k) {
        const int i = (c->slot0 + k) / cfg->nt, j = (c->slot0 + k) % cfg->nt;
        const double Pi = (double)cfg->P[i], Tj = (double)cfg->T[j];
        if (cfg->element != NM_EL_LJ) { // units metal, remcmc:124-127
            const double kb = 8.61733e-5;
            c->h_et[k] = kb * Tj;
            c->h_pf[k] = 1e-30 * (1e5 * Pi) / (1.60218e-19 * kb * Tj);
        } else {                        // remcmc:128-131
            const double kb = 1.0;
            c->h_et[k] = kb * Tj;
            c->h_pf[k] = Pi / (kb * Tj);
        }
        c->h_tq[k] = Tj;
    }

    // size class: the first kind whose configurations hold N atoms (every potential's kind 2 holds the 2048 checked above)
    auto nmax = [&](int kind) { const Row *r = nm_row(c->pot, kind, 1); return r ? r->nmax : 0; };
    for (c->kind = 0; c->kind < 2 && nmax(c->kind) < c->N; ++c->kind) {}
    // the neighbour lists in HBM, per slot: the largest of the kind's rows (a heal can take a 6^3 context from Q = 8, whose lists are in LDS, to Q = 4)
    size_t nbr_elems = 0;
    for (int q : { 1, 2, 4, 8 })
        if (const Row *r = nm_row(c->pot, c->kind, q)) nbr_elems = std::max(nbr_elems, r->nbr_g_elems);

    HIPCHK(c, hipSetDevice(cfg->device));
    HIPCHK(c, c->stream.create());
    set_q(c, 1, false);
    const size_t ns = c->nslots, n3 = (size_t)3 * c->N;
    std::string note;
    {
        int want = 8;
        if (const char *e = std::getenv("NM_CUS_PER_REPLICA")) want = std::atoi(e);
        // what the census probe needs
        HIPCHK(c, c->d_census.alloc(census_words(c->nslots)));
        HIPCHK(c, c->d_status.alloc_zeroed(ns));
        HIPCHK(c, c->d_status_acc.alloc_zeroed(ns));
        HIPCHK(c, c->d_rerun.alloc(ns));
        HIPCHK(c, c->d_order.alloc(ns));
        HIPCHK(c, c->d_last_ticks.alloc_zeroed(ns)); // (first launch: all ties, i.e. index order)
        HIPCHK(c, c->d_halt.alloc_zeroed(1));
        {
            std::vector<int> ident(ns);
            for (int k = 0; k < c->nslots; ++k) ident[k] = k;
            HIPCHK(c, c->d_slot2buf.upload(ident.data(), ns));
        }
        if (const int rc = pick_q(c, want, note)) return rc; // (workgroups per replica: see pick_q)
        if (!note.empty()) note = "nm_create: " + note;
        if (testing())
            if (const char *e = std::getenv("NM_TEST_CENSUS_BASE")) { // tests: start the monotonic census counters just below the value at
                // which issue_block zeroes them (a wrap is otherwise 16 million launches away)
                const unsigned int b = (unsigned int)std::strtoul(e, nullptr, 0);
                std::vector<unsigned int> w(census_words(c->nslots), b);
                HIPCHK(c, hipMemcpy(c->d_census, w.data(), sizeof(unsigned int) * w.size(), hipMemcpyHostToDevice));
                c->census_base = c->census_cbase = b;
            }
        {
            hipDeviceProp_t prop;
            HIPCHK(c, hipGetDeviceProperties(&prop, cfg->device));
            c->use_order = c->over || c->nslots > prop.multiProcessorCount; // (more workgroups / clusters than the chip holds at once: longest first)
            if (const char *e = std::getenv("NM_LAUNCH_ORDER")) c->use_order = std::atoi(e) != 0;
        }
    }
    HIPCHK(c, c->d_x.alloc_zeroed(ns * n3)); HIPCHK(c, c->d_v.alloc_zeroed(ns * n3));
    HIPCHK(c, c->d_box.alloc_zeroed(ns)); HIPCHK(c, c->d_steps.alloc_zeroed(ns * 3)); HIPCHK(c, c->d_therm.alloc_zeroed(ns * 5));
    HIPCHK(c, c->d_count.alloc_zeroed(ns * 6)); HIPCHK(c, c->d_ratio.alloc_zeroed(ns * 3));
    HIPCHK(c, c->d_et.upload(c->h_et.data(), ns)); HIPCHK(c, c->d_pf.upload(c->h_pf.data(), ns)); HIPCHK(c, c->d_tq.upload(c->h_tq.data(), ns));
    HIPCHK(c, c->d_stats.alloc_zeroed(ns * NM_STATS_COLS));
    HIPCHK(c, c->d_nswaps.alloc_zeroed(1)); // (the allocations stand in the order they always had: where a buffer lies is not free)
    HIPCHK(c, c->d_evalU.alloc(ns)); HIPCHK(c, c->d_evalW.alloc(ns)); HIPCHK(c, c->d_evalF.alloc(ns * n3));
    const int npairs = c->cfg.nrows * cfg->nt * (cfg->nt - 1) / 2;
    HIPCHK(c, c->d_xcrit.alloc((size_t)npairs)); HIPCHK(c, c->d_xtape.alloc((size_t)npairs));
#ifdef NM_EXPERIMENT
    HIPCHK(c, c->d_tline.alloc_zeroed((size_t)8 * 8 * 512 * 8));
#endif
#ifdef NM_PROF
    HIPCHK(c, c->d_prof.alloc_zeroed(ns * 16));
#endif
    if (nbr_elems) HIPCHK(c, c->d_nbr.alloc(ns * 2 * nbr_elems)); // two lists per slot (Cfg::LIST2)
    if (const int rc = alloc_cluster_buffers(c)) return rc;
    for (int q : { 1, 2, 4, 8 })
        if (const Row *r = nm_row(c->pot, c->kind, q)) HIPCHK(c, r->request_lds());
    c->ev.resize(32);
    for (auto &e : c->ev) { HIPCHK(c, e.a.create()); HIPCHK(c, e.b.create()); }
    c->note = note; // nm_create_note(ctx): what the residency probe had to give up, if anything
    return NM_OK;
}

int nm_create(const nm_config *cfg, nm_ctx **out)
{
    if (!cfg || !out) return fail(nullptr, NM_ERR_ARG, "nm_create: null argument");
    *out = nullptr;
    if (cfg->size != (int32_t)sizeof(nm_config)) return fail(nullptr, NM_ERR_ARG, "nm_create: nm_config size mismatch (ABI)");
    if (cfg->natoms < 2 || cfg->natoms > 2048) return fail(nullptr, NM_ERR_ARG, "nm_create: natoms must be in [2, 2048]");
    const bool by_slots = cfg->nslots > 0;
    if (cfg->np < 1 || cfg->nt < 1) return fail(nullptr, NM_ERR_ARG, "nm_create: bad grid");
    if (by_slots ? (cfg->slot0 < 0 || cfg->slot0 + cfg->nslots > cfg->np * cfg->nt)
                 : (cfg->nrows < 1 || cfg->row0 < 0 || cfg->row0 + cfg->nrows > cfg->np))
        return fail(nullptr, NM_ERR_ARG, "nm_create: bad row / slot range");
    if (!cfg->P || !cfg->T) return fail(nullptr, NM_ERR_ARG, "nm_create: P and T grids are required");
    if (cfg->nstps < 1 || cfg->ppos < 0 || cfg->pvol < 0 || cfg->ppos + cfg->pvol > 1.0)
        return fail(nullptr, NM_ERR_ARG, "nm_create: bad move parameters");
    if (cfg->element != NM_EL_LJ && !lat::sc_element(cfg->element))
        return fail(nullptr, NM_ERR_UNSUPPORTED, "nm_create: elements LJ (0), Al (1), Ni (2) and Cu (3) have device force kernels in this build");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, NM_ERR_HIP, "nm_create: no HIP device available (this engine has no CPU fallback)");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(nullptr, NM_ERR_ARG, "nm_create: device ordinal out of range");

    std::unique_ptr<nm_ctx> c(new nm_ctx());
    if (init_ctx(c.get(), cfg) != NM_OK) { // (every failure in there is a HIP call's)
        g_create_error = c->err;
        return NM_ERR_HIP;
    }
    *out = c.release();
    return NM_OK;
}

int nm_destroy(nm_ctx *c)
{
    if (!c) return NM_ERR_ARG;
    hipSetDevice(c->cfg.device);
    delete c;
    return NM_OK;
}

int nm_get_const(const nm_ctx *c, double *et, double *pf)
{
    if (!c) return NM_ERR_ARG;
    if (et) std::memcpy(et, c->h_et.data(), sizeof(double) * c->nslots);
    if (pf) std::memcpy(pf, c->h_pf.data(), sizeof(double) * c->nslots);
    return NM_OK;
}

int nm_set_step(nm_ctx *c, uint32_t step)
{
    if (!c) return NM_ERR_ARG;
    c->step = step;
    return NM_OK;
}

int nm_set_state(nm_ctx *c, int k0, int nk, const double *x, const double *v, const double *box, const double *dxdvdt)
{
    if (!c || k0 < 0 || nk < 0 || k0 + nk > c->nslots) return fail(c, NM_ERR_ARG, "nm_set_state: slot range");
    return copy_range(c, true, k0, nk, const_cast<double *>(x), const_cast<double *>(v), const_cast<double *>(box), const_cast<double *>(dxdvdt));
}

int nm_get_state(nm_ctx *c, int k0, int nk, double *x, double *v, double *box, double *dxdvdt)
{
    if (!c || k0 < 0 || nk < 0 || k0 + nk > c->nslots) return fail(c, NM_ERR_ARG, "nm_get_state: slot range");
    return copy_range(c, false, k0, nk, x, v, box, dxdvdt);
}

int nm_get_slots(nm_ctx *c, int nk, const int *slots, double *x, double *v, double *box, double *dxdvdt, double *th)
{
    return copy_list(c, "nm_get_slots", false, nk, slots, x, v, box, dxdvdt, th);
}

int nm_set_slots(nm_ctx *c, int nk, const int *slots, const double *x, const double *v, const double *box, const double *dxdvdt,
                 const double *th)
{
    return copy_list(c, "nm_set_slots", true, nk, slots, const_cast<double *>(x), const_cast<double *>(v), const_cast<double *>(box),
                     const_cast<double *>(dxdvdt), const_cast<double *>(th));
}

int nm_init_lattice(nm_ctx *c, double dx, double dv, int interpolate)
{
    if (!c) return NM_ERR_ARG;
    int sz = 1;
    while (4 * sz * sz * sz < c->N) ++sz;
    if (4 * sz * sz * sz != c->N) return fail(c, NM_ERR_ARG, "nm_init_lattice: natoms is not 4*sz^3 (fcc)");
    const int ns = c->nslots, nt = c->cfg.nt;
    const size_t n3 = (size_t)3 * c->N;
    std::vector<double> frac, x((size_t)ns * n3), v((size_t)ns * n3, 0.0), box((size_t)ns), d((size_t)3 * ns);
    lat::fcc_fractional(sz, frac);
    double brow = 0.0;
    int row = -1;
    for (int k = 0; k < ns; ++k) {
        const int g = c->slot0 + k, i = g / nt, j = g % nt;
        if (i != row) { brow = lat::relax_box(c->cfg.element, sz, (double)c->cfg.P[i]); row = i; }
        lat::init_state(c->cfg.element, sz, brow, c->cfg.seed, g, j, nt, dx, interpolate, frac, x.data() + (size_t)k * n3, &box[k]);
        d[3 * k] = dx; d[3 * k + 1] = dv; d[3 * k + 2] = 0.00390625; // TIMESTEP, remcmc:891-893 (lj and metal)
    }
    return nm_set_state(c, 0, ns, x.data(), v.data(), box.data(), d.data());
}

int nm_set_thermo(nm_ctx *c, int k0, int nk, const double *th)
{
    if (!c || !th || k0 < 0 || nk < 0 || k0 + nk > c->nslots) return fail(c, NM_ERR_ARG, "nm_set_thermo: bad argument");
    std::vector<int> m;
    if (const int rc = slot_map(c, m)) return rc;
    for (int q = 0; q < nk; ++q)
        HIPCHK(c, hipMemcpy(c->d_therm + 5 * (size_t)m[k0 + q], th + 5 * q, 5 * sizeof(double), hipMemcpyHostToDevice));
    return NM_OK;
}

// ---- recorded cycles and output snapshots: write_outputs (remcmc:259-286) without stopping the stream.  A record holds what a recorded cycle writes
// (the 17 thermo columns, the box and the positions of every slot) as of the point of the queue where it is taken.  The records of one call fill a
// ring on the device, one D2H on the side stream brings the ring to pinned host memory behind the call's last record while the main stream goes on,
// and nm_snapshot_fetch hands the records out one by one, oldest first, waiting for that ring's copy only.  nm_run_cycles_recorded takes a record
// behind each of its cycles into ring 0 or 1; nm_snapshot, queued right behind nm_run_block (in front of nm_adapt, which zeroes the counters), takes
// one into ring 2 or 3 — two of each, so that a driver fetches cycle s - 1 after it has queued cycle s.  (nm_get_thermo + nm_get_state, the
// synchronous way, stop the GPU between two blocks for the copies and the host's turn-around: 7 % of a recorded C2 run.)  A record carries a tag
// (call, cycle) that only a block which completed writes: a record whose tag is wrong was not taken (its block stopped, or was re-issued behind the
// copy), and the fetch then settles the queue — which re-issues a launch that can be healed, into the same ring — and copies the ring again.
static const size_t REC_BUDGET = (size_t)64 << 20; // bytes of one call ring: 64 cycles of the 8 x 8 grid at 256 atoms (26 MB), 5 of 1024 x 500 atoms

static int record_capacity(const nm_ctx *c)
{
    const size_t per = rec_cycle_doubles(c) * sizeof(double);
    return (int)std::max<size_t>(1, std::min<size_t>(64, REC_BUDGET / per));
}

// rings r0 and r0 + 1 of cap cycles each, and the side stream if there is none: all or nothing
static int ring_alloc(nm_ctx *c, int r0, int cap, const char *who)
{
    const size_t nd = (size_t)cap * rec_cycle_doubles(c);
    Stream side;
    nm_ctx::Ring g[2];
    hipError_t e = c->side ? hipSuccess : side.create();
    for (auto &q : g) {
        if (e == hipSuccess) e = q.d.alloc(nd);
        if (e == hipSuccess) e = q.h.alloc(nd);
        if (e == hipSuccess) e = q.taken.create(hipEventDisableTiming);
        if (e == hipSuccess) e = q.landed.create(hipEventDisableTiming);
        q.cap = cap;
    }
    if (e != hipSuccess) return fail(c, NM_ERR_HIP, std::string(who) + ": ring allocation: " + hipGetErrorString(e)); // (the locals take all of it back)
    if (side) c->side = std::move(side);
    c->ring[r0] = std::move(g[0]); c->ring[r0 + 1] = std::move(g[1]);
    return NM_OK;
}

// the records of one call go to the free ring r: a fresh tag, set before they are issued
static void open_ring(nm_ctx *c, int r)
{
    c->ring[r].tag0 = ((++c->rec_calls & 0xFFFFFFu) << 7) + 1; // (a record left from an earlier call of this ring never matches)
    c->ring[r].dirty = false;
}

// behind the n records just issued into ring r: one D2H on the side stream, and the records join the fetch queue
static int land_ring(nm_ctx *c, int r, int n)
{
    nm_ctx::Ring &g = c->ring[r];
    HIPCHK(c, hipEventRecord(g.taken, c->stream));
    HIPCHK(c, hipStreamWaitEvent(c->side, g.taken, 0));
    HIPCHK(c, hipMemcpyAsync(g.h, g.d, (size_t)n * rec_cycle_doubles(c) * sizeof(double), hipMemcpyDeviceToHost, c->side));
    HIPCHK(c, hipEventRecord(g.landed, c->side));
    g.n = n; g.next = 0;
    for (int k = 0; k < n; ++k) c->fetchq.push_back(r);
    return NM_OK;
}

int nm_snapshot(nm_ctx *c)
{
    if (!c) return NM_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    const int r = c->ring[2].n == 0 ? 2 : c->ring[3].n == 0 ? 3 : -1;
    if (r < 0) return fail(c, NM_ERR_STATE, "nm_snapshot: two snapshots are pending; fetch one first (nm_snapshot_fetch)");
    if (!c->ring[2].cap) {
        const int rc = ring_alloc(c, 2, 1, "nm_snapshot");
        if (rc) return rc;
    }
    open_ring(c, r);
    const int rc = issue_record(c, r, 0);
    return rc ? rc : land_ring(c, r, 1);
}

// the records of ring r still queued are dropped (a fetch that reports an error)
static void drop_ring(nm_ctx *c, int r)
{
    c->ring[r].n = c->ring[r].next = 0;
    c->fetchq.erase(std::remove(c->fetchq.begin(), c->fetchq.end(), r), c->fetchq.end());
}

static int fetch_record(nm_ctx *c, int r, double *rows, double *x, double *box)
{
    nm_ctx::Ring &g = c->ring[r];
    HIPCHK(c, hipEventSynchronize(g.landed));
    const size_t n3 = (size_t)3 * c->N, rs = n3 + NM_REC_HEAD, ns = c->nslots;
    const int j = g.next;
    const double *const rec = g.h + (size_t)j * rec_cycle_doubles(c);
    const double tag = (double)(g.tag0 + (uint32_t)j);
    auto taken = [&]() {
        for (size_t k = 0; k < ns; ++k)
            if (rec[k * rs + NM_REC_TAG] != tag) return false;
        return true;
    };
    if (g.dirty || !taken()) {
        const int rc = check_status(c); // the queue's outcome: a healable stop is re-issued (into this ring), an error is reported
        if (rc) { drop_ring(c, r); return rc; }
        HIPCHK(c, hipMemcpy(g.h, g.d, (size_t)g.n * rec_cycle_doubles(c) * sizeof(double), hipMemcpyDeviceToHost));
        g.dirty = false;
        if (!taken()) {
            drop_ring(c, r);
            return fail(c, NM_ERR_STATE, "nm_snapshot_fetch: a snapshot or recorded cycle was never taken (the block in front of it did not complete)");
        }
    }
    for (size_t k = 0; k < ns; ++k) {
        const double *s = rec + k * rs;
        if (rows) std::memcpy(rows + k * NM_THERMO_COLS, s, NM_THERMO_COLS * sizeof(double));
        if (x) std::memcpy(x + k * n3, s + NM_REC_HEAD, n3 * sizeof(double));
        if (box) box[k] = s[NM_REC_BOX];
    }
    c->fetchq.pop_front();
    if (++g.next == g.n) g.n = g.next = 0;
    return NM_OK;
}

int nm_snapshot_fetch(nm_ctx *c, double *rows, double *x, double *box)
{
    if (!c) return NM_ERR_ARG;
    if (c->fetchq.empty()) return fail(c, NM_ERR_STATE, "nm_snapshot_fetch: no snapshot is pending");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    return fetch_record(c, c->fetchq.front(), rows, x, box);
}

int nm_record_capacity(const nm_ctx *c) { return c ? record_capacity(c) : NM_ERR_ARG; }
int nm_snapshot_pending(const nm_ctx *c) { return c ? (int)c->fetchq.size() : NM_ERR_ARG; }

int nm_run_cycles_recorded(nm_ctx *c, int ncycles, int mod)
{
    if (!c || ncycles < 1 || mod < 0) return fail(c, NM_ERR_ARG, "nm_run_cycles_recorded: bad argument");
    if (!c->whole_rows) return fail(c, NM_ERR_UNSUPPORTED, "nm_run_cycles_recorded: this context holds a partial pressure row (the exchange spans contexts)");
    if (ncycles > record_capacity(c))
        return fail(c, NM_ERR_ARG, "nm_run_cycles_recorded: " + std::to_string(ncycles) + " cycles, more than one call holds (nm_record_capacity: " +
                                       std::to_string(record_capacity(c)) + ")");
    const int r = c->ring[0].n == 0 ? 0 : c->ring[1].n == 0 ? 1 : -1;
    if (r < 0) return fail(c, NM_ERR_STATE, "nm_run_cycles_recorded: the records of two calls are pending; fetch them first (nm_snapshot_fetch)");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (!c->ring[0].cap) {
        const int rc = ring_alloc(c, 0, record_capacity(c), "nm_run_cycles_recorded");
        if (rc) return rc;
    }
    open_ring(c, r);
    const int rc = issue_cycles(c, ncycles, mod, c->step, true, r, 0);
    return rc ? rc : land_ring(c, r, ncycles);
}

int nm_run_block(nm_ctx *c, int mod)
{
    if (!c || mod < 0) return fail(c, NM_ERR_ARG, "nm_run_block: bad argument");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    return issue_block(c, OP_BLOCK, mod, c->step, c->trace_on, nullptr, true);
}

int nm_run_md(nm_ctx *c, int nsteps)
{
    if (!c || nsteps < 1) return fail(c, NM_ERR_ARG, "nm_run_md: bad argument");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    return issue_block(c, OP_MD, nsteps, c->step, 0, nullptr, false);
}

int nm_run_cycles(nm_ctx *c, int ncycles, int mod)
{
    if (!c || ncycles < 1 || mod < 0) return fail(c, NM_ERR_ARG, "nm_run_cycles: bad argument");
    if (!c->whole_rows) return fail(c, NM_ERR_UNSUPPORTED, "nm_run_cycles: this context holds a partial pressure row (the exchange spans contexts)");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    return issue_cycles(c, ncycles, mod, c->step, true, -1, 0);
}

int nm_get_thermo(nm_ctx *c, double *rows)
{
    if (!c || !rows) return fail(c, NM_ERR_ARG, "nm_get_thermo: null argument");
    std::vector<int> m;
    if (const int rc = slot_map(c, m)) return rc;
    const size_t ns = c->nslots;
    std::vector<double> th(ns * 5), st(ns * 3), cn(ns * 6);
    std::vector<float> ra(ns * 3);
    HIPCHK(c, hipMemcpy(th.data(), c->d_therm, th.size() * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(st.data(), c->d_steps, st.size() * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(cn.data(), c->d_count, cn.size() * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(ra.data(), c->d_ratio, ra.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < ns; ++k) {
        const int b = m[k];
        double *r = rows + k * NM_THERMO_COLS;
        r[0] = th[5 * b]; r[1] = th[5 * b + 1]; r[2] = th[5 * b + 2]; r[3] = th[5 * b + 3]; r[4] = th[5 * b + 4];
        r[5] = st[3 * b]; r[6] = st[3 * b + 1]; r[7] = st[3 * b + 2];
        for (int q = 0; q < 6; ++q) r[8 + q] = cn[6 * k + q];
        for (int q = 0; q < 3; ++q) r[14 + q] = (double)ra[3 * k + q];
    }
    return NM_OK; // (slot_map has looked at the outcome of everything queued)
}

int nm_adapt(nm_ctx *c)
{
    if (!c) return NM_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    return issue_adapt(c);
}

int nm_exchange(nm_ctx *c, int *nswaps)
{
    if (!c) return NM_ERR_ARG;
    if (!c->whole_rows)
        return fail(c, NM_ERR_UNSUPPORTED, "nm_exchange: this context holds a partial pressure row; the sweep spans contexts (host exchange over RCCL)");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    int rc = issue_exchange(c, c->step);
    if (rc) return rc;
    if (nswaps) {
        if ((rc = check_status(c))) return rc;
        HIPCHK(c, hipMemcpy(nswaps, c->d_nswaps, sizeof(int), hipMemcpyDeviceToHost));
    }
    return NM_OK;
}

int nm_synchronize(nm_ctx *c)
{
    if (!c) return NM_ERR_ARG;
    return settled(c);
}

int nm_get_status(nm_ctx *c, int *status)
{
    if (!c || !status) return fail(c, NM_ERR_ARG, "nm_get_status: null argument");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    (void)check_status(c); // re-issues a halted queue; an error that cannot be cured leaves its bits in d_status (settle), which is what this call is for
    HIPCHK(c, hipMemcpy(status, c->d_status, sizeof(int) * c->nslots, hipMemcpyDeviceToHost));
    return NM_OK;
}

int nm_timing_reset(nm_ctx *c)
{
    if (!c) return NM_ERR_ARG;
    for (auto &e : c->ev) harvest(c, e);
    c->launches = 0; c->total_ms = 0.0;
    return NM_OK;
}

int nm_timing_get(nm_ctx *c, int *launches, double *total_ms)
{
    if (!c) return NM_ERR_ARG;
    for (auto &e : c->ev) harvest(c, e);
    if (launches) *launches = c->launches;
    if (total_ms) *total_ms = c->total_ms;
    return NM_OK;
}

int nm_stats_get(nm_ctx *c, double *stats, int reset)
{
    if (!c || !stats) return fail(c, NM_ERR_ARG, "nm_stats_get: null argument");
    if (const int rc = settled(c)) return rc;
    const size_t n = (size_t)c->nslots * NM_STATS_COLS;
    HIPCHK(c, hipMemcpy(stats, c->d_stats, n * sizeof(double), hipMemcpyDeviceToHost));
    if (reset) HIPCHK(c, hipMemset(c->d_stats, 0, n * sizeof(double)));
    return NM_OK;
}

#ifdef NM_EXPERIMENT
int nm_tline_get(nm_ctx *c, unsigned long long *out)
{
    if (!c || !out) return NM_ERR_ARG;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, c->d_tline, (size_t)8 * 8 * 512 * 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return NM_OK;
}
#endif
#ifdef NM_PROF
// diagnostic build only: out-of-range indices into the global spill / list arrays since the last call (counted and redirected by
// the kernel, nm_kernels.h NM_CHECK_INDEX); scripts/check_bounds.py runs the large-cell parity cases under it
int nm_prof_oob(nm_ctx *c, unsigned int *count)
{
    if (!c || !count) return NM_ERR_ARG;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, prof_take_count(0, count));
    return NM_OK;
}
// diagnostic build only: rows of freshly built neighbour lists that lacked an atom inside rc + skin (exact fp64 check after every
// rebuild, Replica::rebuild) since the last call
int nm_prof_list_miss(nm_ctx *c, unsigned int *count)
{
    if (!c || !count) return NM_ERR_ARG;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, prof_take_count(1, count));
    return NM_OK;
}
int nm_prof_miss_info(nm_ctx *c, double *info16)
{
    if (!c || !info16) return NM_ERR_ARG;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, prof_miss_info(info16));
    return NM_OK;
}
// diagnostic build only: cycle sums per section and slot, [nslots][16]
int nm_prof_get(nm_ctx *c, unsigned long long *out, int reset)
{
    if (!c || !out) return NM_ERR_ARG;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, c->d_prof, (size_t)c->nslots * 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    if (reset) HIPCHK(c, hipMemset(c->d_prof, 0, (size_t)c->nslots * 16 * sizeof(unsigned long long)));
    return NM_OK;
}
#endif

int nm_eval(nm_ctx *c, double *U, double *W, double *f)
{
    if (!c || !U || !W) return fail(c, NM_ERR_ARG, "nm_eval: null argument");
    if (const int rc = settled(c)) return rc; // (whatever is queued first: an evaluation is not re-issued)
    ++c->launch_id;
    KParams p;
    fill_params(c, p);
    p.eval_only = 1; p.tape = nullptr;
    p.evalU = c->d_evalU; p.evalW = c->d_evalW; p.evalF = f ? c->d_evalF : nullptr;
    HIPCHK(c, launch_kind(c, p));
    census_advance(c);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t ns = c->nslots;
    HIPCHK(c, hipMemcpy(U, c->d_evalU, ns * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(W, c->d_evalW, ns * sizeof(double), hipMemcpyDeviceToHost));
    if (f) HIPCHK(c, hipMemcpy(f, c->d_evalF, ns * 3 * c->N * sizeof(double), hipMemcpyDeviceToHost));
    return check_status(c);
}

int nm_set_rng_tape(nm_ctx *c, const double *tape, const int *offsets)
{
    if (!c) return NM_ERR_ARG;
    if (const int rc = settled(c)) return rc;
    c->d_tape = {}; c->d_tape_off = {}; // (the tape that was set goes in any case)
    if (!tape || !offsets) return NM_OK;
    const int total = offsets[c->nslots];
    if (total < 0) return fail(c, NM_ERR_ARG, "nm_set_rng_tape: bad offsets");
    DevBuf<double> t;
    DevBuf<int> off;
    HIPCHK(c, t.upload(tape, (size_t)total));
    HIPCHK(c, off.upload(offsets, (size_t)c->nslots + 1));
    c->d_tape = std::move(t); c->d_tape_off = std::move(off);
    return NM_OK;
}

int nm_set_exchange_tape(nm_ctx *c, const double *tape, int n)
{
    if (!c) return NM_ERR_ARG;
    if (const int rc = settled(c)) return rc;
    const int npairs = c->cfg.nrows * c->cfg.nt * (c->cfg.nt - 1) / 2;
    if (!tape) { c->xtape_n = 0; return NM_OK; }
    if (n != npairs) return fail(c, NM_ERR_ARG, "nm_set_exchange_tape: need one uniform per pair of the sweep");
    HIPCHK(c, hipMemcpy(c->d_xtape, tape, sizeof(double) * n, hipMemcpyHostToDevice));
    c->xtape_n = n;
    return NM_OK;
}

int nm_set_trace(nm_ctx *c, int enable)
{
    if (!c) return NM_ERR_ARG;
    c->trace_on = enable ? 1 : 0;
    return NM_OK;
}

int nm_get_trace(nm_ctx *c, double *trace, int mod)
{
    if (!c || !trace) return fail(c, NM_ERR_ARG, "nm_get_trace: null argument");
    if (!c->d_trace || mod != c->trace_mod) return fail(c, NM_ERR_ARG, "nm_get_trace: no trace of that length recorded");
    if (const int rc = settled(c)) return rc;
    HIPCHK(c, hipMemcpy(trace, c->d_trace, (size_t)c->nslots * mod * NM_TRACE_COLS * sizeof(double), hipMemcpyDeviceToHost));
    return NM_OK;
}

int nm_set_counters(nm_ctx *c, const double *count, const float *ratio)
{
    if (!c) return NM_ERR_ARG;
    if (const int rc = settled(c)) return rc;
    if (count) HIPCHK(c, hipMemcpy(c->d_count, count, sizeof(double) * 6 * c->nslots, hipMemcpyHostToDevice));
    if (ratio) HIPCHK(c, hipMemcpy(c->d_ratio, ratio, sizeof(float) * 3 * c->nslots, hipMemcpyHostToDevice));
    return NM_OK;
}

int nm_get_perm(nm_ctx *c, int *perm)
{
    if (!c || !perm) return fail(c, NM_ERR_ARG, "nm_get_perm: null argument");
    if (const int rc = settled(c)) return rc;
    HIPCHK(c, hipMemcpy(perm, c->d_slot2buf, sizeof(int) * c->nslots, hipMemcpyDeviceToHost));
    return NM_OK;
}

int nm_get_exchange_crit(nm_ctx *c, double *crit, int n)
{
    if (!c || !crit) return fail(c, NM_ERR_ARG, "nm_get_exchange_crit: null argument");
    const int npairs = c->cfg.nrows * c->cfg.nt * (c->cfg.nt - 1) / 2;
    if (n != npairs) return fail(c, NM_ERR_ARG, "nm_get_exchange_crit: wrong pair count");
    if (const int rc = settled(c)) return rc;
    HIPCHK(c, hipMemcpy(crit, c->d_xcrit, sizeof(double) * n, hipMemcpyDeviceToHost));
    return NM_OK;
}

} // extern "C"
