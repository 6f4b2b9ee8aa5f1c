// nm_io.cpp — the entry points that are plain host code: output formatting and the context-free lattice state of include/nm.h,
// and the .thrm / .traj reader of include/nm_parse.h.  No HIP header comes in here, so this file compiles without the device pass.
#include "../../include/nm.h"
#include "../../include/nm_parse.h"
#include "nm_format.h"
#include "nm_lattice.h"
#include "nm_parse.h"

#include <cstdio>
#include <string>
#include <thread>
#include <vector>

using namespace nm;

// the message behind nm_last_error(NULL), defined with the sampler (nm_api.hip)
namespace nm { extern __attribute__((visibility("hidden"))) thread_local std::string g_create_error; }

// ---------------------------------------------------------------------------------------------------------------
// output formatting (include/nm.h; write_outputs, remcmc:235-286): plain host code
extern "C" {

int nm_format_thrm(const double *row17, char *out, int cap)
{
    if (!row17 || !out || cap < 17 * 14 + 2) return NM_ERR_ARG;
    return format_thrm(row17, out);
}

int nm_format_traj(int natoms, double box, const double *x, char *out, int cap)
{
    if (natoms < 0 || !x || !out || cap < 32 + 42 * natoms) return NM_ERR_ARG;
    return format_traj(natoms, box, x, out);
}

int nm_append_outputs(int nk, int natoms, const char *const *thrm_paths, const char *const *traj_paths, const double *rows,
                      const double *x, const double *box, int nthreads)
{
    if (nk < 0 || natoms < 0 || !thrm_paths || !traj_paths || !rows || !x || !box) return NM_ERR_ARG;
    if (nthreads <= 0) nthreads = (int)std::thread::hardware_concurrency();
    if (nthreads < 1) nthreads = 1;
    if (nthreads > nk) nthreads = nk > 0 ? nk : 1;
    std::vector<int> err((size_t)nthreads, 0);
    auto work = [&](int t) {
        std::vector<char> buf((size_t)64 + 42 * (size_t)natoms + 17 * 14);
        for (int k = t; k < nk; k += nthreads) {
            int n = format_thrm(rows + 17 * (size_t)k, buf.data());
            FILE *f = std::fopen(thrm_paths[k], "a");
            if (!f || std::fwrite(buf.data(), 1, (size_t)n, f) != (size_t)n) err[t] = 1;
            if (f) std::fclose(f);
            n = format_traj(natoms, box[k], x + 3 * (size_t)natoms * k, buf.data());
            f = std::fopen(traj_paths[k], "a");
            if (!f || std::fwrite(buf.data(), 1, (size_t)n, f) != (size_t)n) err[t] = 1;
            if (f) std::fclose(f);
        }
    };
    std::vector<std::thread> th;
    for (int t = 1; t < nthreads; ++t) th.emplace_back(work, t);
    work(0);
    for (auto &t : th) t.join();
    for (int e : err) if (e) return NM_ERR_ARG;
    return NM_OK;
}

} // extern "C"

int nm_lattice_state(int element, int sz, int np, int nt, const float *P, uint32_t seed, int gslot, double dx, int interpolate, double *x,
                     double *box)
{
    if ((element != NM_EL_LJ && !lat::sc_element(element)) || sz < 1 || np < 1 || nt < 1 || !P || gslot < 0 || gslot >= np * nt || !x || !box)
    {
        g_create_error = "nm_lattice_state: bad argument";
        return NM_ERR_ARG;
    }
    std::vector<double> frac;
    lat::fcc_fractional(sz, frac);
    const double b = lat::relax_box(element, sz, (double)P[gslot / nt]);
    lat::init_state(element, sz, b, seed, gslot, gslot % nt, nt, dx, interpolate, frac, x, box);
    return NM_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// .thrm / .traj reader (include/nm_parse.h; lammps_parse.py:48-49, 88-96)
// ------------------------------------------------------------------------------------------------------------------
namespace {
thread_local std::string g_parse_error;
}
extern "C" {
const char *nm_parse_last_error(void) { return g_parse_error.c_str(); }

int nm_parse_thrm(const char *path, float *rows, long cap_rows, long *nrows, int nthreads)
{
    if (!path || (rows && cap_rows < 0)) { g_parse_error = "nm_parse_thrm: bad argument"; return NM_ERR_ARG; }
    try {
        return nm::parse_thrm(path, rows, cap_rows, nrows, nthreads, g_parse_error) == 0 ? NM_OK : NM_ERR_ARG;
    } catch (const std::exception &e) { g_parse_error = e.what(); return NM_ERR_ARG; }
}

int nm_parse_traj(const char *path, uint16_t *natoms, float *box, float *pos, long cap_frames, long cap_posrows, long *nframes,
                  long *nposrows, int nthreads)
{
    if (!path) { g_parse_error = "nm_parse_traj: bad argument"; return NM_ERR_ARG; }
    try {
        return nm::parse_traj(path, natoms, box, pos, cap_frames, cap_posrows, nframes, nposrows, nthreads, g_parse_error) == 0
                   ? NM_OK : NM_ERR_ARG;
    } catch (const std::exception &e) { g_parse_error = e.what(); return NM_ERR_ARG; }
}
}
