// lmi_host_fetch.h -- lmi_rows_fetch / lmi_rows_fetch_f16: stored objects by id, the geometry hook and the plan words (kernels:
// lmi_fetch.h; the arithmetic: lmi_fetch_plan.h; include/lmi_hip.h states the contract).
// No reference counterpart on the device: the reference answers `data_search.loc[ids]` from a DataFrame it keeps on the host
// (LearnedIndex.py:357); a resident index has no such frame, and lmi_bucket_read needs the bucket.
// A call: the request list is sorted and de-duplicated on the host (ids on the device are copied down first: 4n bytes, the call's one
// internal synchronisation), the tables go up (at most 16n bytes, freed before the call returns), one pass over ids_slab locates every
// id, then one gather per piece of requests.  Host outputs go through h->stage piece by piece (what 64 MiB hold); device outputs are
// written in place, 2^24 requests per launch.  The location table (8 bytes per distinct id) is copied down ahead of the closing
// synchronisation, for device outputs too: FOUND of lmi_debug_fetch_plan is counted from it on the host.
// The call only reads the index: clone views, derived handles and sharded ranks are served alike.
#pragma once
#include "lmi_host_call.h"
#include "lmi_fetch.h"
#include "lmi_fetch_plan.h"

static_assert(FETCH_FRAG32 == FORM_FRAG32 && FETCH_ROWMAJOR == FORM_ROWMAJOR && FETCH_FRAG16 == FORM_FRAG16,
              "lmi_fetch.h spells the stored forms as numbers");

namespace {

thread_local int64_t g_fetch_piece_rows = 0;   // 0: what a 64-MiB stage holds (lmi_fetch_plan::piece_rows_for)
thread_local int64_t g_fetch_last[LMI_FETCH_PLAN_COUNT] = {};

struct FetchCall {
    const char* who;
    bool half;
    int on_device;
    void* rows;
    int32_t *bucket, *row;
};

// the gather of requests [c0, c0 + pn) into rows / bucket / row (device pointers of THAT piece; each nullable)
int fetch_gather(lmi_index* h, bool half, const unsigned long long* d_loc, const int* d_map, int64_t c0, int64_t pn, void* rows, int* bucket,
                 int* row) {
    const StoredForm form = stored_form(h);
    const int du = h->d_user, nc = fetch_piece_cols((int)form);
    FetchSource S{};
    S.rb_start = h->d_rb_start.as<int>();
    S.d = du;
    switch (form) {
    case FORM_FRAG32: S.image = h->slab.p, S.pitch = h->KGs; break;
    case FORM_ROWMAJOR: S.image = h->rowmajor.p, S.pitch = h->dp; break;
    case FORM_FRAG16: S.image = h->slab16.p, S.pitch = h->KG16, S.f16x16 = frag16x16(h), S.scale = h->xscale.as<float>(); break;
    }
    const int vec = rows && du % nc == 0 && (reinterpret_cast<uintptr_t>(rows) & 15) == 0;
    const long long lanes = (long long)pn * (rows ? cdiv(du, nc) : 1);
    const dim3 grid((unsigned)cdiv(lanes, 256));
    unsigned* flag = h->rd_flag.as<unsigned>();
#define LMI_FETCH_LAUNCH(FORM, HALF) \
    fetch_gather_kernel<FORM, HALF><<<grid, 256, 0, h->stream>>>(S, d_loc, d_map, c0, pn, rows, bucket, row, vec, flag)
    switch (form) {
    case FORM_FRAG32: if (half) LMI_FETCH_LAUNCH(FETCH_FRAG32, true); else LMI_FETCH_LAUNCH(FETCH_FRAG32, false); break;
    case FORM_ROWMAJOR: if (half) LMI_FETCH_LAUNCH(FETCH_ROWMAJOR, true); else LMI_FETCH_LAUNCH(FETCH_ROWMAJOR, false); break;
    case FORM_FRAG16: if (half) LMI_FETCH_LAUNCH(FETCH_FRAG16, true); else LMI_FETCH_LAUNCH(FETCH_FRAG16, false); break;
    }
#undef LMI_FETCH_LAUNCH
    HIPCHK(hipGetLastError());
    return 0;
}

// whether a narrowing gather raised the flag: one word down, one synchronisation
int fetch_flag(lmi_index* h, const char* who) {
    unsigned bad = 0;
    HIPCHK(hipMemcpyAsync(&bad, h->rd_flag.p, 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (bad)
        return fail("%s: a fetched value is not exactly representable in binary16 (or not finite); nothing was returned -- fetch it with "
                    "lmi_rows_fetch", who);
    return 0;
}

// everything behind the refusals and the plan, n > 0; on failure the caller synchronises before the tables free themselves and before
// the plan's vectors, which the uploads read, go
int fetch_run(lmi_index* h, const lmi_fetch_plan::Plan& P, const FetchCall& C, CallScratch& mem, std::vector<unsigned long long>& h_loc) {
    namespace fp = lmi_fetch_plan;
    hipStream_t st = h->stream;
    const int du = h->d_user;
    const size_t elt = C.half ? 2 : 4;
    const int64_t n = P.n;
    const size_t nu = P.unique.size();
    uint32_t* d_unique = nullptr;
    int* d_map = nullptr;
    unsigned long long* d_loc = nullptr;
    CHK(mem.alloc(&d_unique, nu * 4, "sorted ids"));
    CHK(mem.alloc(&d_map, (size_t)n * 4, "request map"));
    CHK(mem.alloc(&d_loc, nu * 8, "location table"));
    HIPCHK(hipMemcpyAsync(d_unique, P.unique.data(), nu * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_map, P.map.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(d_loc, 0xff, nu * 8, st));
    const int max_n = h->L > 0 ? *std::max_element(h->h_nb_rows.begin(), h->h_nb_rows.end()) : 0;
    if (max_n > 0) {
        fetch_locate_kernel<<<dim3(std::max(1, std::min(64, cdiv(max_n, 256))), h->L), 256, 0, st>>>(
            h->ids_slab.as<uint32_t>(), h->d_rb_start.as<int>(), h->d_nb_rows.as<int>(), d_unique, (int)nu, d_loc);
        HIPCHK(hipGetLastError());
    }
    const bool narrowing = C.half && C.rows && stored_form(h) != FORM_FRAG16;
    if (narrowing) {
        CHK(h->rd_flag.reserve(16));
        HIPCHK(hipMemsetAsync(h->rd_flag.p, 0, 4, st));
    }
    const int64_t pieces = P.pieces();
    size_t stage_bytes = 0;
    if (C.on_device) {
        for (int64_t p = 0; p < pieces; ++p) {
            const int64_t c0 = P.piece_begin(p), pn = P.piece_end(p) - c0;
            CHK(fetch_gather(h, C.half, d_loc, d_map, c0, pn, C.rows ? static_cast<char*>(C.rows) + (size_t)c0 * du * elt : nullptr,
                             C.bucket ? C.bucket + c0 : nullptr, C.row ? C.row + c0 : nullptr));
        }
        if (narrowing) CHK(fetch_flag(h, C.who));
    } else {
        // a piece's stage: [rows pn x du, rounded up to 16 bytes | bucket pn | row pn]
        const int64_t stage_rows = std::min(P.piece_rows, n);
        const size_t rows_bytes = C.rows ? (size_t)rup((long long)stage_rows * du * (long long)elt, 16) : 0;
        stage_bytes = rows_bytes + (size_t)stage_rows * 8;
        CHK(h->stage.reserve(stage_bytes));
        char* s_rows = h->stage.as<char>();
        int* s_bucket = reinterpret_cast<int*>(s_rows + rows_bytes);
        int* s_row = s_bucket + stage_rows;
        // a host output receives nothing from a call that fails: where the verdict of a later piece could come after an earlier
        // piece's copy, every piece is gathered once for the verdict alone, then again for the copies
        if (narrowing && pieces > 1) {
            for (int64_t p = 0; p < pieces; ++p)
                CHK(fetch_gather(h, true, d_loc, d_map, P.piece_begin(p), P.piece_end(p) - P.piece_begin(p), s_rows, nullptr, nullptr));
            CHK(fetch_flag(h, C.who));
        }
        for (int64_t p = 0; p < pieces; ++p) {
            const int64_t c0 = P.piece_begin(p), pn = P.piece_end(p) - c0;
            CHK(fetch_gather(h, C.half, d_loc, d_map, c0, pn, C.rows ? s_rows : nullptr, C.bucket ? s_bucket : nullptr, C.row ? s_row : nullptr));
            if (narrowing && pieces == 1) CHK(fetch_flag(h, C.who));
            if (C.rows) HIPCHK(hipMemcpyAsync(static_cast<char*>(C.rows) + (size_t)c0 * du * elt, s_rows, (size_t)pn * du * elt, hipMemcpyDeviceToHost, st));
            if (C.bucket) HIPCHK(hipMemcpyAsync(C.bucket + c0, s_bucket, (size_t)pn * 4, hipMemcpyDeviceToHost, st));
            if (C.row) HIPCHK(hipMemcpyAsync(C.row + c0, s_row, (size_t)pn * 4, hipMemcpyDeviceToHost, st));
            // (the next piece's gather overwrites the stage behind these copies, in stream order)
        }
    }
    // FOUND is counted on the host: the location table (8 bytes per distinct id) comes down ahead of the call's closing synchronisation
    h_loc.resize(nu);
    HIPCHK(hipMemcpyAsync(h_loc.data(), d_loc, nu * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    int64_t found = 0;
    for (int64_t i = 0; i < n; ++i) found += h_loc[(size_t)P.map[(size_t)i]] != fp::ABSENT;
    g_fetch_last[LMI_FETCH_PLAN_REQUESTS] = n;
    g_fetch_last[LMI_FETCH_PLAN_UNIQUE] = (int64_t)nu;
    g_fetch_last[LMI_FETCH_PLAN_PIECES] = pieces;
    g_fetch_last[LMI_FETCH_PLAN_PIECE_ROWS] = P.piece_rows;
    g_fetch_last[LMI_FETCH_PLAN_FOUND] = found;
    g_fetch_last[LMI_FETCH_PLAN_WORKSPACE_BYTES] = mem.total + (int64_t)stage_bytes;
    return 0;
}

int fetch_impl(lmi_index* h, const uint32_t* ids, int64_t n, const FetchCall& C) {
    const char* who = C.who;
    for (int64_t& w : g_fetch_last) w = 0;
    if (!h) return fail("%s: NULL handle", who);
    if (!h->built) return fail("%s: the bucket index is not built", who);
    if (!lmi_fetch_plan::n_ok(n)) return fail("%s: n = %lld outside [0, 2^31)", who, (long long)n);
    if (n > 0 && !ids) return fail("%s: ids is NULL", who);
    if (!C.rows && !C.bucket && !C.row) return fail("%s: rows, bucket and row are all NULL: nothing was asked for", who);
    g_fetch_last[LMI_FETCH_PLAN_FORM] = (int64_t)stored_form(h);
    if (n == 0) return 0;
    namespace fp = lmi_fetch_plan;
    CHK(set_dev(h));
    std::vector<uint32_t> h_ids;
    if (C.on_device) {   // the list is sorted on the host: 4n bytes down, the call's one internal synchronisation
        h_ids.resize((size_t)n);
        HIPCHK(hipMemcpyAsync(h_ids.data(), ids, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        ids = h_ids.data();
    }
    const fp::Plan P = fp::make_plan(ids, n, fp::piece_rows_for(g_fetch_piece_rows, fp::request_bytes(h->d_user, C.half ? 2 : 4, C.rows != nullptr),
                                                                !C.on_device));
    std::vector<unsigned long long> h_loc;
    CallScratch mem(who);
    if (fetch_run(h, P, C, mem, h_loc) != 0) {
        (void)hipStreamSynchronize(h->stream);   // no kernel may still read the tables that free themselves
        for (int64_t& w : g_fetch_last) w = 0;
        return -1;
    }
    return 0;
}

}  // namespace

extern "C" LMI_API int lmi_fetch_set_geometry(int64_t piece_rows) {
    if (!lmi_fetch_plan::piece_rows_ok(piece_rows))
        return fail("lmi_fetch_set_geometry: piece_rows %lld outside [0, 2^24]", (long long)piece_rows);
    g_fetch_piece_rows = piece_rows;
    return 0;
}

extern "C" LMI_API int lmi_debug_fetch_plan(int64_t* out, int n) {
    if (!out || n < 0) return fail("lmi_debug_fetch_plan: NULL argument");
    for (int i = 0; i < std::min(n, (int)LMI_FETCH_PLAN_COUNT); ++i) out[i] = g_fetch_last[i];
    return 0;
}

extern "C" LMI_API int lmi_rows_fetch(lmi_index* h, const uint32_t* ids, int64_t n, float* rows, int32_t* bucket, int32_t* row, int on_device) {
    return fetch_impl(h, ids, n, FetchCall{"lmi_rows_fetch", false, on_device, rows, bucket, row});
}
extern "C" LMI_API int lmi_rows_fetch_f16(lmi_index* h, const uint32_t* ids, int64_t n, uint16_t* rows, int32_t* bucket, int32_t* row,
                                          int on_device) {
    return fetch_impl(h, ids, n, FetchCall{"lmi_rows_fetch_f16", true, on_device, rows, bucket, row});
}
