// nm_host.h — the host scaffold of the offline stages (nm_distr_api.hip, nm_reweight_api.hip, nm_pca_api.hip, nm_cluster_api.hip):
// the stage's error channel with its HIP check and device selection, and the rest of a batch; the device memory that frees itself is
// nm_own.h's, which the sampler shares.  Internal: every name here has internal linkage, so each stage gets its own copy and its own message.
#pragma once
#include "../../include/nm.h"

#include "nm_own.h"

#include <cstdint>
#include <string>

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

} // namespace
