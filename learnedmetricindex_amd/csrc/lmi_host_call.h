// lmi_host_call.h -- the frame of a call that needs no handle (lmi_kmeans, lmi_train, lmi_knn; lmi_create opens its device the same
// way): the device, the call's own device allocations, the upload of host memory on the NULL stream.
#pragma once
#include "lmi_handle.h"
#include <algorithm>

namespace {

// device in range, current, and a gfx950: `who` names the call in the messages
int open_device(const char* who, int device, hipDeviceProp_t* prop) {
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail("%s: device %d out of range (%d devices)", who, device, ndev);
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipGetDeviceProperties(prop, device));
    if (std::string(prop->gcnArchName).rfind("gfx950", 0) != 0)
        return fail("%s: device %d is %s; this library is built for gfx950 only", who, device, prop->gcnArchName);
    return 0;
}

// the device allocations of one call, each of exactly the bytes asked for: freed when the call returns, whichever way
struct CallScratch {
    const char* who;
    std::vector<void*> owned;
    int64_t total = 0;   // bytes asked for so far
    explicit CallScratch(const char* who_) : who(who_) {}
    CallScratch(const CallScratch&) = delete;
    ~CallScratch() { for (void* p : owned) (void)hipFree(p); }
    template <class T>
    int alloc(T** out, size_t bytes, const char* what) {
        void* p = nullptr;
        if (hipError_t e = hipMalloc(&p, bytes ? bytes : 4); e != hipSuccess) {
            (void)hipGetLastError();
            return fail("%s: a device allocation of %zu bytes (%s) failed: %s", who, bytes, what, hipGetErrorString(e));
        }
        owned.push_back(p);
        total += (int64_t)bytes;
        *out = static_cast<T*>(p);
        return 0;
    }
};

// host memory goes up in 64-MiB pieces, on the NULL stream
int upload_pieces(void* dst, const void* src, size_t bytes) {
    const size_t piece = (size_t)64 << 20;
    for (size_t o = 0; o < bytes; o += piece)
        HIPCHK(hipMemcpyAsync(static_cast<char*>(dst) + o, static_cast<const char*>(src) + o, std::min(piece, bytes - o),
                              hipMemcpyHostToDevice, nullptr));
    return 0;
}

}  // namespace
