// lmi_host_comm.h -- the exchange step of the bucket-sharded mode: lmi_merge_gathered and the RCCL calls (lmi_comm_*, lmi_allgather_merge);
// for the union scan lmi_merge_union_parts and lmi_allgather_merge_union (the kernel: lmi_union_merge.h).
#pragma once
#include "lmi_host.h"
#include "lmi_union_merge.h"
#include <dlfcn.h>
#include <mutex>
#include <rccl/rccl.h>  // types only: the functions are resolved at run time (lmi_comm_*), the library does not link RCCL

extern "C" LMI_API int lmi_merge_gathered(lmi_index* h, const float* gd, const uint32_t* gi, const uint32_t* gk, int world,
                                  int64_t world_stride, int nq, int kout, float* dists, uint32_t* ids,
                                  int on_device) {
    if (!h) return fail("lmi_merge_gathered: NULL handle");
    if (world < 1 || world > 64) return fail("lmi_merge_gathered: world %d outside [1,64]", world);
    if (nq <= 0 || kout < 1) return nq == 0 ? 0 : fail("lmi_merge_gathered: bad nq/kout");
    CHK(set_dev(h));
    const size_t nin = (size_t)world * nq * kout * 4, nout = (size_t)nq * kout * 4;
    if (world_stride == 0) world_stride = (int64_t)nq * kout;
    if (on_device) {
        merge_gathered_kernel<<<nq, 64, 0, h->stream>>>(gd, gi, gk, world, world_stride, nq, kout, dists, ids);
        HIPCHK(hipGetLastError());
        return 0;
    }
    if (world_stride != (int64_t)nq * kout) return fail("lmi_merge_gathered: host buffers must be dense (world_stride 0)");
    DevBuf in, out;
    CHK(in.reserve(3 * nin));
    CHK(out.reserve(2 * nout));
    char* ip = in.as<char>();
    HIPCHK(hipMemcpyAsync(ip, gd, nin, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(ip + nin, gi, nin, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(ip + 2 * nin, gk, nin, hipMemcpyHostToDevice, h->stream));
    merge_gathered_kernel<<<nq, 64, 0, h->stream>>>(reinterpret_cast<float*>(ip), reinterpret_cast<unsigned*>(ip + nin),
                                                   reinterpret_cast<unsigned*>(ip + 2 * nin), world, world_stride, nq, kout,
                                                   out.as<float>(), reinterpret_cast<unsigned*>(out.as<char>() + nout));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(dists, out.p, nout, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(ids, out.as<char>() + nout, nout, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;   // (in and out free themselves, on the early returns above too)
}

namespace {
// what both merges of union parts refuse before any launch; *go <- whether there is anything to do
int union_merge_check(const char* who, lmi_index* h, int world, int nq, int k, bool* go) {
    *go = false;
    if (!h) return fail("%s: NULL handle", who);
    if (world < 1 || world > 64) return fail("%s: world %d outside [1,64]", who, world);
    if (k < 1 || k > LMI_UNION_MAX_K) return fail("%s: k %d outside [1,%d]", who, k, LMI_UNION_MAX_K);
    if (nq < 0) return fail("%s: nq %d is negative", who, nq);
    if ((long long)world * LMI_UNION_PART_PLANES * nq * k >= (1ll << 31)) return fail("%s: world*5*nq*k too large", who);
    *go = nq > 0;
    return 0;
}
int union_merge_launch(lmi_index* h, const int* parts, int world, int nq, int k, float* dists, unsigned* ids, int* counts) {
    int LR = 128;   // lmi_union_plan::list_rows_for(k)
    while (LR < k) LR <<= 1;
    union_merge_kernel<<<nq, 64, (size_t)4 * LR * 8, h->stream>>>(parts, world, nq, k, LR, dists, ids, counts);
    HIPCHK(hipGetLastError());
    return 0;
}
}  // namespace

extern "C" LMI_API int lmi_merge_union_parts(lmi_index* h, const int32_t* parts, int world, int nq, int k, float* dists, uint32_t* ids,
                                             int32_t* counts, int on_device) {
    const char* who = "lmi_merge_union_parts";
    bool go = false;
    CHK(union_merge_check(who, h, world, nq, k, &go));
    if (!go) return 0;
    if (!parts || !dists || !ids) return fail("%s: parts, dists and ids must not be NULL", who);
    CHK(set_dev(h));
    if (on_device) return union_merge_launch(h, parts, world, nq, k, dists, ids, counts);
    const size_t nin = (size_t)world * LMI_UNION_PART_PLANES * nq * k * 4, nout = (size_t)nq * k * 4;
    DevBuf in, out;
    CHK(in.reserve(nin));
    CHK(out.reserve(2 * nout + (size_t)nq * 4));
    float* d_D = out.as<float>();
    unsigned* d_I = reinterpret_cast<unsigned*>(out.as<char>() + nout);
    int* d_C = reinterpret_cast<int*>(out.as<char>() + 2 * nout);
    HIPCHK(hipMemcpyAsync(in.p, parts, nin, hipMemcpyHostToDevice, h->stream));
    CHK(union_merge_launch(h, in.as<int>(), world, nq, k, d_D, d_I, d_C));
    HIPCHK(hipMemcpyAsync(dists, d_D, nout, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(ids, d_I, nout, hipMemcpyDeviceToHost, h->stream));
    if (counts) HIPCHK(hipMemcpyAsync(counts, d_C, (size_t)nq * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;   // (in and out free themselves, on the early returns above too)
}

// ---- RCCL (resolved from the process image -- PyTorch-ROCm has it loaded -- or from librccl.so) ----------------
namespace {
struct Rccl {
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    bool ok = false;
};
Rccl* rccl() {
    static Rccl r;
    static std::once_flag once;
    std::call_once(once, [] {
        void* lib = RTLD_DEFAULT;
        if (!dlsym(lib, "ncclAllGather")) {
            for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so"})
                if ((lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL))) break;
            if (!lib) return;
        }
        r.GetUniqueId = reinterpret_cast<decltype(r.GetUniqueId)>(dlsym(lib, "ncclGetUniqueId"));
        r.CommInitRank = reinterpret_cast<decltype(r.CommInitRank)>(dlsym(lib, "ncclCommInitRank"));
        r.CommDestroy = reinterpret_cast<decltype(r.CommDestroy)>(dlsym(lib, "ncclCommDestroy"));
        r.AllGather = reinterpret_cast<decltype(r.AllGather)>(dlsym(lib, "ncclAllGather"));
        r.GetErrorString = reinterpret_cast<decltype(r.GetErrorString)>(dlsym(lib, "ncclGetErrorString"));
        r.ok = r.GetUniqueId && r.CommInitRank && r.CommDestroy && r.AllGather;
    });
    return &r;
}
int rccl_fail(const char* what, ncclResult_t e) {
    Rccl* r = rccl();
    return fail("%s failed: %s", what, r->GetErrorString ? r->GetErrorString(e) : "RCCL error");
}
}  // namespace

extern "C" LMI_API int lmi_comm_unique_id(void* id128) {
    if (!id128) return fail("lmi_comm_unique_id: NULL buffer");
    if (!rccl()->ok) return fail("lmi_comm_unique_id: RCCL (librccl.so) is not available in this process");
    ncclUniqueId id;
    ncclResult_t e = rccl()->GetUniqueId(&id);
    if (e != ncclSuccess) return rccl_fail("ncclGetUniqueId", e);
    memcpy(id128, &id, sizeof(id));
    return 0;
}

extern "C" LMI_API int lmi_comm_init(lmi_index* h, int rank, int world, const void* id128, void** comm) {
    if (!h || !id128 || !comm) return fail("lmi_comm_init: NULL argument");
    if (world < 1 || world > 64 || rank < 0 || rank >= world) return fail("lmi_comm_init: rank %d of %d", rank, world);
    if (!rccl()->ok) return fail("lmi_comm_init: RCCL (librccl.so) is not available in this process");
    CHK(set_dev(h));
    ncclUniqueId id;
    memcpy(&id, id128, sizeof(id));
    ncclComm_t c = nullptr;
    ncclResult_t e = rccl()->CommInitRank(&c, world, id, rank);
    if (e != ncclSuccess) return rccl_fail("ncclCommInitRank", e);
    *comm = c;
    return 0;
}

extern "C" LMI_API int lmi_comm_destroy(void* comm) {
    if (!comm) return 0;
    if (!rccl()->ok) return fail("lmi_comm_destroy: RCCL is not available");
    ncclResult_t e = rccl()->CommDestroy(static_cast<ncclComm_t>(comm));
    return e == ncclSuccess ? 0 : rccl_fail("ncclCommDestroy", e);
}

// The exchange step of the bucket-sharded mode through the C ABI alone: this rank's lmi_scan_topk /
// lmi_search outputs (device pointers, [nq][kout] each) -> ONE ncclAllGather of the packed [dists | ids | keys] block
// over `comm` on the handle's stream -> merge_gathered_kernel -> dists / ids [nq][kout] (device), identical on
// every rank and to the single-GPU result.
extern "C" LMI_API int lmi_allgather_merge(lmi_index* h, void* comm, int rank, int world, const float* local_dists,
                                   const uint32_t* local_ids, const uint32_t* local_keys, int nq, int kout, float* dists,
                                   uint32_t* ids) {
    if (!h || !comm) return fail("lmi_allgather_merge: NULL handle/communicator");
    if (world < 1 || world > 64 || rank < 0 || rank >= world) return fail("lmi_allgather_merge: rank %d of %d", rank, world);
    if (nq <= 0 || kout < 1) return nq == 0 ? 0 : fail("lmi_allgather_merge: bad nq/kout");
    if (!rccl()->ok) return fail("lmi_allgather_merge: RCCL (librccl.so) is not available in this process");
    CHK(set_dev(h));
    const size_t plane = (size_t)nq * kout;
    CHK(h->gather_send.reserve(3 * plane * 4));
    CHK(h->gather_recv.reserve((size_t)world * 3 * plane * 4));
    char* snd = h->gather_send.as<char>();
    HIPCHK(hipMemcpyAsync(snd, local_dists, plane * 4, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(snd + plane * 4, local_ids, plane * 4, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(snd + 2 * plane * 4, local_keys, plane * 4, hipMemcpyDeviceToDevice, h->stream));
    ncclResult_t e = rccl()->AllGather(snd, h->gather_recv.p, 3 * plane, ncclInt32, static_cast<ncclComm_t>(comm), h->stream);
    if (e != ncclSuccess) return rccl_fail("ncclAllGather", e);
    const char* rcv = h->gather_recv.as<char>();
    merge_gathered_kernel<<<nq, 64, 0, h->stream>>>(reinterpret_cast<const float*>(rcv), reinterpret_cast<const unsigned*>(rcv + plane * 4),
                                                   reinterpret_cast<const unsigned*>(rcv + 2 * plane * 4), world, (long long)(3 * plane),
                                                   nq, kout, dists, ids);
    HIPCHK(hipGetLastError());
    return 0;
}

// The union scan's exchange: this rank's part (lmi_scan_union_part, a device pointer) -> ONE ncclAllGather of its 5 * nq * k words over
// `comm` on the handle's stream -> union_merge_kernel -> dists / ids [nq][k], counts [nq] (device), identical on every rank.
extern "C" LMI_API int lmi_allgather_merge_union(lmi_index* h, void* comm, int rank, int world, const int32_t* part, int nq, int k,
                                                 float* dists, uint32_t* ids, int32_t* counts) {
    const char* who = "lmi_allgather_merge_union";
    bool go = false;
    CHK(union_merge_check(who, h, world, nq, k, &go));
    if (!comm) return fail("%s: NULL communicator", who);
    if (rank < 0 || rank >= world) return fail("%s: rank %d of %d", who, rank, world);
    if (!go) return 0;
    if (!part || !dists || !ids) return fail("%s: part, dists and ids must not be NULL", who);
    if (!rccl()->ok) return fail("%s: RCCL (librccl.so) is not available in this process", who);
    CHK(set_dev(h));
    const size_t words = (size_t)LMI_UNION_PART_PLANES * nq * k;
    CHK(h->gather_send.reserve(words * 4));
    CHK(h->gather_recv.reserve((size_t)world * words * 4));
    HIPCHK(hipMemcpyAsync(h->gather_send.p, part, words * 4, hipMemcpyDeviceToDevice, h->stream));
    ncclResult_t e = rccl()->AllGather(h->gather_send.p, h->gather_recv.p, words, ncclInt32, static_cast<ncclComm_t>(comm), h->stream);
    if (e != ncclSuccess) return rccl_fail("ncclAllGather", e);
    return union_merge_launch(h, h->gather_recv.as<int>(), world, nq, k, dists, ids, counts);
}
