// nm_host.h — the host scaffold of the offline stages (nm_distr_api.hip, nm_reweight_api.hip, nm_pca_api.hip, nm_cluster_api.hip, nm_tsne_api.hip):
// the stage's error channel with its HIP check and device selection, the rest of a batch, the screen of a host array for values
// that are not finite and the lap timer behind nm_*_last_timing; the device memory and the events that free themselves are
// nm_own.h's, which the sampler shares; the all-pairs scan of the cluster and the manifold stage, grid and tables included, is
// nm_scan.h's.  Internal: every name here has internal linkage, so each stage gets its own copy and its own message.
#pragma once
#include "../../include/nm.h"

#include "nm_own.h"

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

namespace {

// The message behind the stage's nm_*_last_error: each stage defines this over a thread_local string of its own file, so that
// a failure in one stage leaves the other's message alone.
std::string &stage_error();

int fail(int code, const std::string &m) { stage_error() = m; return code; }
int refuse(const char *fn, const char *why) { return fail(NM_ERR_ARG, std::string(fn) + ": " + why); }

// a failed HIP call ends the entry point `fn` with NM_ERR_HIP; what it allocated is freed by the buffers' destructors
#define STAGE_CHK(fn, call)                                                                                            \
    do {                                                                                                               \
        hipError_t e_ = (call);                                                                                        \
        if (e_ != hipSuccess) return fail(NM_ERR_HIP, std::string(fn) + ": " + #call + ": " + hipGetErrorString(e_)); \
    } while (0)

// makes `device` the calling thread's device.  A negative ordinal is refused before a device is looked for: it is the
// last of an entry point's NM_ERR_ARG that needs none
int stage_device(const char *fn, int device)
{
    if (device < 0) return refuse(fn, "device ordinal out of range");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(NM_ERR_HIP, std::string(fn) + ": no HIP device available");
    if (device >= ndev) return refuse(fn, "device ordinal out of range");
    STAGE_CHK(fn, hipSetDevice(device));
    return NM_OK;
}

// how many of n items the batch that starts at t0 holds: `batch`, or what is left of n
int batch_rest(int n, int t0, int64_t batch) { return (n - t0) < batch ? (n - t0) : (int)batch; }

// the index of the first of x[0 .. n - 1] that is not finite, or -1
template <class T> int64_t first_not_finite(const T *x, int64_t n)
{
    for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite(x[i])) return i;
    return -1;
}

// Where a call's device time went, for the stage's nm_*_last_timing: lap(w) books the time since the lap before to slot w of the
// stage's N.  An event that cannot be created only loses that lap.
template <int N> struct Laps {
    std::vector<Event> ev;
    std::vector<int> what;
    void lap(int w)
    {
        Event e;
        if (e.create() != hipSuccess) return;
        hipEventRecord(e, 0);
        ev.push_back(std::move(e));
        what.push_back(w);
    }
    // behind the call's last synchronisation
    void book(double *ms)
    {
        for (int i = 0; i < N; ++i) ms[i] = 0.0;
        for (size_t i = 1; i < ev.size(); ++i) {
            float t = 0.0f;
            if (hipEventElapsedTime(&t, ev[i - 1], ev[i]) == hipSuccess) ms[what[i]] += t;
        }
    }
};

// a stage's nm_*_last_timing: the slots that the last call of this thread booked
template <int N> int last_timing(const char *fn, const double (&booked)[N], double *ms)
{
    if (!ms) return refuse(fn, "a needed pointer is null");
    for (int i = 0; i < N; ++i) ms[i] = booked[i];
    return NM_OK;
}

} // namespace
