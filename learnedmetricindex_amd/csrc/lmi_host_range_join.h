// lmi_host_range_join.h -- the range search across the ranks of a bucket-sharded index: the join of the ranks' parts
// (lmi_join_range_parts), the same behind an exchange through RCCL (lmi_allgather_join_range), the piece-size hook and the plan words
// (kernel: lmi_range_join.h; the arithmetic: lmi_range_join_plan.h; include/lmi_hip.h states the contract).  A part is what
// lmi_scan_range returns on a rank's handle; the joined result is an lmi_range_result like any other.
#pragma once
#include "lmi_host_comm.h"
#include "lmi_host_range.h"
#include "lmi_range_join.h"
#include "lmi_range_join_plan.h"

namespace {

thread_local int64_t g_range_join_piece_rows = 0;   // 0: lmi_range_join_plan::DEFAULT_PIECE_ROWS
thread_local int64_t g_range_join_last[LMI_RANGE_JOIN_COUNT] = {};

// what both joins refuse of their scalar arguments, before any launch or allocation
int range_join_check(const char* who, lmi_index* h, int world, int nq, int nb, int64_t max_total, lmi_range_result** out) {
    for (int64_t& w : g_range_join_last) w = 0;
    if (out) *out = nullptr;
    if (!h) return fail("%s: NULL handle", who);
    if (world < 1 || world > 64) return fail("%s: world %d outside [1,64]", who, world);
    if (nq < 0) return fail("%s: nq %d is negative", who, nq);
    if (nb < 1 || nb > 1024) return fail("%s: nb %d outside [1,1024]", who, nb);
    if ((long long)nq * nb >= (1ll << 31)) return fail("%s: nq*nb too large", who);
    if (!out) return fail("%s: the result pointer is NULL", who);
    if (max_total < 0) return fail("%s: max_total %lld is negative", who, (long long)max_total);
    return 0;
}

// counts -> plan, or the refusal by name
int range_join_plan(const char* who, int world, int nq, int nb, const int32_t* counts, int64_t max_total, lmi_range_join_plan::Plan& P) {
    namespace jp = lmi_range_join_plan;
    const jp::Verdict v = jp::make_plan(world, nq, nb, counts, g_range_join_piece_rows, max_total, P);
    switch (v.problem) {
    case jp::OK: break;
    case jp::NEGATIVE_COUNT:
        return fail("%s: the count of part %d at query %lld, t %d is negative (%lld)", who, v.part_a, (long long)v.q, v.t, (long long)v.value);
    case jp::TWO_OWNERS:
        return fail("%s: query %lld, t %d has results in part %d and in part %d: the parts' buckets overlap (every bucket must be owned by "
                    "exactly one part)", who, (long long)v.q, v.t, v.part_a, v.part_b);
    case jp::OVER_TOTAL:
        return fail("%s: more than max_total = %lld results: the parts hold %lld; nothing was launched", who, (long long)max_total,
                    (long long)v.value);
    }
    if ((long long)P.piece_n.size() >= (1ll << 31)) return fail("%s: %zu copy pieces are more than one launch takes", who, P.piece_n.size());
    return 0;
}

// The join proper: d_dists / d_ids [world] are DEVICE pointers (NULL where the part is empty), already valid on h->stream.  Returns
// when the result is complete.
int range_join_run(lmi_index* h, const char* who, const lmi_range_join_plan::Plan& P, const float* const* d_dists,
                   const uint32_t* const* d_ids, lmi_range_result** out) {
    hipStream_t st = h->stream;
    lmi_range_result* r = new lmi_range_result();
    r->device = h->device;
    r->lims = P.lims;
    r->nb = P.nb;
    r->pair_count = P.pair_count;
    auto run = [&]() -> int {
        if (P.total == 0) return 0;
        HIPCHK(hipMalloc(reinterpret_cast<void**>(&r->dists), (size_t)P.total * 4));
        HIPCHK(hipMalloc(reinterpret_cast<void**>(&r->ids), (size_t)P.total * 4));
        const size_t np = P.piece_n.size(), W = (size_t)P.world;
        CallScratch mem(who);
        const float** t_d = nullptr;
        const unsigned** t_i = nullptr;
        int *p_part = nullptr, *p_n = nullptr;
        long long *p_src = nullptr, *p_dst = nullptr;
        CHK(mem.alloc(&t_d, W * sizeof(void*), "part pointers (dists)"));
        CHK(mem.alloc(&t_i, W * sizeof(void*), "part pointers (ids)"));
        CHK(mem.alloc(&p_part, np * 4, "piece parts"));
        CHK(mem.alloc(&p_n, np * 4, "piece lengths"));
        CHK(mem.alloc(&p_src, np * 8, "piece sources"));
        CHK(mem.alloc(&p_dst, np * 8, "piece targets"));
        HIPCHK(hipMemcpyAsync(t_d, d_dists, W * sizeof(void*), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(t_i, d_ids, W * sizeof(void*), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(p_part, P.piece_part.data(), np * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(p_n, P.piece_n.data(), np * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(p_src, P.piece_src.data(), np * 8, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(p_dst, P.piece_dst.data(), np * 8, hipMemcpyHostToDevice, st));
        range_join_kernel<<<(unsigned)np, RANGE_JOIN_BLOCK, 0, st>>>(t_d, t_i, p_part, p_src, p_dst, p_n, r->dists, r->ids);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(st));   // the result is complete; the tables (and a caller's staged parts) may go
        return 0;
    };
    if (run() != 0) {
        (void)hipStreamSynchronize(st);
        delete r;
        return -1;
    }
    g_range_join_last[LMI_RANGE_JOIN_PARTS] = P.world;
    g_range_join_last[LMI_RANGE_JOIN_RUNS] = P.runs;
    g_range_join_last[LMI_RANGE_JOIN_PIECES] = (int64_t)P.piece_n.size();
    g_range_join_last[LMI_RANGE_JOIN_RESULTS] = P.total;
    g_range_join_last[LMI_RANGE_JOIN_LARGEST_PART] = P.largest_part;
    *out = r;
    return 0;
}

}  // namespace

extern "C" LMI_API int lmi_range_join_set_geometry(int64_t piece_rows) {
    if (piece_rows < 0 || piece_rows > lmi_range_join_plan::MAX_PIECE_ROWS)
        return fail("lmi_range_join_set_geometry: piece_rows %lld outside [0, 2^30]", (long long)piece_rows);
    g_range_join_piece_rows = piece_rows;
    return 0;
}

extern "C" LMI_API int lmi_debug_range_join_plan(int64_t* out, int n) {
    if (!out || n < 0) return fail("lmi_debug_range_join_plan: NULL argument");
    for (int i = 0; i < std::min(n, (int)LMI_RANGE_JOIN_COUNT); ++i) out[i] = g_range_join_last[i];
    return 0;
}

extern "C" LMI_API int lmi_join_range_parts(lmi_index* h, int world, int nq, int nb, const int32_t* counts, const float* const* dists,
                                            const uint32_t* const* ids, int64_t max_total, lmi_range_result** result, int on_device) {
    const char* who = "lmi_join_range_parts";
    CHK(range_join_check(who, h, world, nq, nb, max_total, result));
    if (nq == 0) return range_empty(h, 0, nb, result);
    if (!counts || !dists || !ids) return fail("%s: counts, dists and ids must not be NULL", who);
    lmi_range_join_plan::Plan P;
    CHK(range_join_plan(who, world, nq, nb, counts, max_total, P));
    for (int r = 0; r < world; ++r)
        if (P.part_total[(size_t)r] > 0 && (!dists[r] || !ids[r]))
            return fail("%s: part %d holds %lld results and its dists or ids pointer is NULL", who, r, (long long)P.part_total[(size_t)r]);
    CHK(set_dev(h));
    if (on_device) return range_join_run(h, who, P, dists, ids, result);
    // host parts: each part's arrays are uploaded once, into one staging block [dists of part 0 | ids of part 0 | dists of part 1 | ..]
    int64_t words = 0;
    for (int64_t t : P.part_total) words += 2 * t;
    DevBuf stage;
    CHK(stage.reserve((size_t)std::max<int64_t>(words, 1) * 4));
    std::vector<const float*> sd((size_t)world, nullptr);
    std::vector<const uint32_t*> si((size_t)world, nullptr);
    char* at = stage.as<char>();
    for (int r = 0; r < world; ++r) {
        const size_t bytes = (size_t)P.part_total[(size_t)r] * 4;
        if (bytes == 0) continue;
        HIPCHK(hipMemcpyAsync(at, dists[r], bytes, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(at + bytes, ids[r], bytes, hipMemcpyHostToDevice, h->stream));
        sd[(size_t)r] = reinterpret_cast<const float*>(at);
        si[(size_t)r] = reinterpret_cast<const uint32_t*>(at + bytes);
        at += 2 * bytes;
    }
    const int rc = range_join_run(h, who, P, sd.data(), si.data(), result);
    if (rc != 0) (void)hipStreamSynchronize(h->stream);   // the staging block frees itself: no copy may still be reading into it
    return rc;
}

// The exchange inside the library.  ONE ncclAllGather of the nq * nb counts -> ONE stream synchronisation (the host sizes the payload
// and plans the join from the gathered counts) -> ONE ncclAllGather of [dists | ids] padded to the largest part's total -> the join.
extern "C" LMI_API int lmi_allgather_join_range(lmi_index* h, void* comm, int rank, int world, const lmi_range_result* part,
                                                int64_t max_total, lmi_range_result** result) {
    const char* who = "lmi_allgather_join_range";
    const int nq = part ? (int)part->lims.size() - 1 : 0;   // nq and nb are the part's
    const int nb = part ? part->nb : 1;
    CHK(range_join_check(who, h, world, nq, nb, max_total, result));
    if (!part) return fail("%s: NULL part", who);
    if (part->sorted)
        return fail("%s: the part is sorted by distance (lmi_range_result_sort): the join needs its (rank, row) order; sort the joined "
                    "result instead", who);
    if (!comm) return fail("%s: NULL communicator", who);
    if (rank < 0 || rank >= world) return fail("%s: rank %d of %d", who, rank, world);
    if (!rccl()->ok) return fail("%s: RCCL (librccl.so) is not available in this process", who);
    if (nq == 0) return range_empty(h, 0, nb, result);
    CHK(set_dev(h));
    hipStream_t st = h->stream;
    const size_t pairs = (size_t)nq * nb;
    CHK(h->gather_send.reserve(pairs * 4));
    CHK(h->gather_recv.reserve((size_t)world * pairs * 4));
    HIPCHK(hipMemcpyAsync(h->gather_send.p, part->pair_count.data(), pairs * 4, hipMemcpyHostToDevice, st));
    ncclResult_t e = rccl()->AllGather(h->gather_send.p, h->gather_recv.p, pairs, ncclInt32, static_cast<ncclComm_t>(comm), st);
    if (e != ncclSuccess) return rccl_fail("ncclAllGather", e);
    std::vector<int32_t> counts((size_t)world * pairs);
    HIPCHK(hipMemcpyAsync(counts.data(), h->gather_recv.p, counts.size() * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));   // the call's one synchronisation before the join's own: the counts size everything behind it
    lmi_range_join_plan::Plan P;
    CHK(range_join_plan(who, world, nq, nb, counts.data(), max_total, P));
    const int64_t mine = part->lims.back(), tmax = P.largest_part;
    if (P.part_total[(size_t)rank] != mine)
        return fail("%s: the gathered counts give rank %d %lld results, its part holds %lld", who, rank, (long long)P.part_total[(size_t)rank],
                    (long long)mine);
    std::vector<const float*> sd((size_t)world, nullptr);
    std::vector<const uint32_t*> si((size_t)world, nullptr);
    if (tmax > 0) {
        const size_t block = 2 * (size_t)tmax;   // words a rank sends: [dists, padded to tmax | ids, padded to tmax]
        CHK(h->gather_send.reserve(block * 4));
        CHK(h->gather_recv.reserve((size_t)world * block * 4));
        int* snd = h->gather_send.as<int>();
        if (mine > 0) {
            HIPCHK(hipMemcpyAsync(snd, part->dists, (size_t)mine * 4, hipMemcpyDeviceToDevice, st));
            HIPCHK(hipMemcpyAsync(snd + tmax, part->ids, (size_t)mine * 4, hipMemcpyDeviceToDevice, st));
        }
        e = rccl()->AllGather(snd, h->gather_recv.p, block, ncclInt32, static_cast<ncclComm_t>(comm), st);
        if (e != ncclSuccess) return rccl_fail("ncclAllGather", e);
        const int* rcv = h->gather_recv.as<int>();
        for (int r = 0; r < world; ++r) {
            sd[(size_t)r] = reinterpret_cast<const float*>(rcv + (size_t)r * block);
            si[(size_t)r] = reinterpret_cast<const uint32_t*>(rcv + (size_t)r * block + tmax);
        }
    }
    return range_join_run(h, who, P, sd.data(), si.data(), result);
}
