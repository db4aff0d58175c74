// lmi_host_cover.h -- the bucket cover and the exact range search through it (kernels: lmi_cover.h; the rule and the geometry:
// lmi_cover_plan.h; include/lmi_hip.h states the contract): lmi_cover_create / _destroy / _read, lmi_cover_order,
// lmi_search_range_exact, lmi_cover_set_geometry, lmi_debug_cover_plan.
// No reference counterpart (the reference answers a range query from the buckets its model ranks first and has no exact form).
// A cover is made by three passes over the stored rows; it is keyed by the layout stamp as a filter set is (lmi_host_filter.h).
// The pruning pass (CoverPass) takes the queries in groups: per group one admission launch fills the group's bitmap and one compaction
// counts it; the counts of the whole call come down (ONE synchronisation), the host decides nb or refuses, and where an order is
// wanted a second compaction writes it (a call of more than one group judges each group again for it: the bitmap is a group's).
// lmi_search_range_exact hands that order to range_core (lmi_host_range.h), which runs unchanged.
#pragma once
#include "lmi_host_range.h"
#include "lmi_cover.h"
#include "lmi_cover_plan.h"

static_assert(LMI_METRIC_IP == lmi_cover_plan::METRIC_IP && LMI_METRIC_L2 == lmi_cover_plan::METRIC_L2,
              "lmi_cover_plan.h restates the metrics");

// A cover: per bucket the live rows, the centre, the covering radius and the centre's norm, on the device.  It holds no pointer to the
// handle: the stamp says which handles it fits.
struct lmi_cover {
    uint64_t stamp = 0;   // the layout stamp of the handle it was made from
    int device = 0, L = 0, d = 0, metric = 0;
    std::vector<int> nb_rows;   // [L]: the live rows (0: empty, or not owned by this rank)
    float* centres = nullptr;   // [L][d]
    float* radius = nullptr;    // [L]
    double* cn = nullptr;       // [L]
    int* d_nb_rows = nullptr;   // [L]
    int64_t bytes = 0;
    lmi_cover() = default;
    lmi_cover(const lmi_cover&) = delete;
    ~lmi_cover() {
        for (void* p : {(void*)centres, (void*)radius, (void*)cn, (void*)d_nb_rows})
            if (p) (void)hipFree(p);
    }
    template <class T>
    int alloc(T** out, size_t want, const char* what) {
        void* p = nullptr;
        if (hipError_t e = hipMalloc(&p, want ? want : 4); e != hipSuccess) {
            (void)hipGetLastError();
            return fail("lmi_cover_create: a device allocation of %zu bytes (%s) failed: %s", want, what, hipGetErrorString(e));
        }
        *out = static_cast<T*>(p);
        bytes += (int64_t)want;
        return 0;
    }
};

namespace {

thread_local int64_t g_cover_query_rows = 0;   // 0: lmi_cover_plan::query_rows_for's default
thread_local int64_t g_cover_last[LMI_COVER_PLAN_COUNT] = {};

// what every call that takes a cover refuses of it, before any launch
int cover_check(const lmi_index* h, const char* who, const lmi_cover* c) {
    if (!c) return fail("%s: NULL cover", who);
    if (c->stamp != h->layout_stamp || c->device != h->device)
        return fail("%s: the cover is stale or belongs to another index: it was made under layout stamp %llu, this handle carries %llu "
                    "(lmi_buckets_insert / _delete, lmi_subset, lmi_regroup and lmi_concat give a new layout; make the cover again)",
                    who, (unsigned long long)c->stamp, (unsigned long long)h->layout_stamp);
    return 0;
}

// the three passes; everything the call allocates beside the cover's own arrays is `mem`'s
int cover_fill(lmi_index* h, lmi_cover* c, CallScratch& mem) {
    const int L = c->L, d = c->d, dp = h->dp;
    hipStream_t st = h->stream;
    CHK(c->alloc(&c->centres, (size_t)L * d * 4, "centres"));
    CHK(c->alloc(&c->radius, (size_t)L * 4, "radii"));
    CHK(c->alloc(&c->cn, (size_t)L * 8, "centre norms"));
    CHK(c->alloc(&c->d_nb_rows, (size_t)L * 4, "row counts"));
    unsigned long long *d_S = nullptr, *d_r2 = nullptr;
    unsigned* d_max = nullptr;
    CHK(mem.alloc(&d_S, (size_t)L * d * 8, "sums"));
    CHK(mem.alloc(&d_r2, (size_t)L * 8, "squared radii"));
    CHK(mem.alloc(&d_max, 4, "maximum"));
    HIPCHK(hipMemcpyAsync(c->d_nb_rows, c->nb_rows.data(), (size_t)L * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(d_S, 0, (size_t)L * d * 8, st));
    HIPCHK(hipMemsetAsync(d_r2, 0, (size_t)L * 8, st));
    HIPCHK(hipMemsetAsync(d_max, 0, 4, st));
    const int max_n = *std::max_element(c->nb_rows.begin(), c->nb_rows.end());
    const float* rows = h->rowmajor.as<float>();
    const int* rbs = h->d_rb_start.as<int>();
    const int* nbr = h->d_nb_rows.as<int>();
    const bool vec = d % 4 == 0 && dp % 4 == 0;
    const int E = vec ? d / 4 : d;
    const dim3 tiles((unsigned)std::max(1, std::min(4096, cdiv(max_n, COVER_TILE_ROWS))), (unsigned)L);
    unsigned maxbits = 0;
    if (max_n > 0) {
        if (vec) cover_absmax_kernel<true><<<tiles, 256, 0, st>>>(rows, dp, d, rbs, nbr, d_max);
        else cover_absmax_kernel<false><<<tiles, 256, 0, st>>>(rows, dp, d, rbs, nbr, d_max);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&maxbits, d_max, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));   // the exponent of the sums is decided on the host, as lmi_kmeans decides it
    }
    int e = 0;   // the smallest integer with max|x| < 2^e over the finite live values (0 for all-zero data)
    if (maxbits) {
        float m;
        std::memcpy(&m, &maxbits, 4);
        (void)std::frexp((double)m, &e);
    }
    const double scale = std::ldexp(1.0, lmi_cover_plan::SUM_BITS - e), unscale = std::ldexp(1.0, e - lmi_cover_plan::SUM_BITS);
    if (max_n > 0) {
        const dim3 grid(tiles.x, tiles.y, (unsigned)cdiv(E, 256));
        if (vec) cover_accum_kernel<true><<<grid, 256, 0, st>>>(rows, dp, d, rbs, nbr, scale, d_S);
        else cover_accum_kernel<false><<<grid, 256, 0, st>>>(rows, dp, d, rbs, nbr, scale, d_S);
        HIPCHK(hipGetLastError());
    }
    cover_centre_kernel<<<cdiv((long long)L * d, 256), 256, 0, st>>>(reinterpret_cast<const long long*>(d_S), c->d_nb_rows, L, d, unscale, c->centres);
    HIPCHK(hipGetLastError());
    cover_cnorm_kernel<<<cdiv(L, 64), 64, 0, st>>>(c->centres, L, d, c->cn);
    HIPCHK(hipGetLastError());
    if (max_n > 0) {
        const dim3 grid((unsigned)std::max(1, std::min(4096, cdiv(max_n, COVER_RAD_ROWS))), (unsigned)L);
        if (vec) cover_radius_kernel<true><<<grid, COVER_RAD_ROWS, 0, st>>>(rows, dp, d, rbs, nbr, c->centres, d_r2);
        else cover_radius_kernel<false><<<grid, COVER_RAD_ROWS, 0, st>>>(rows, dp, d, rbs, nbr, c->centres, d_r2);
        HIPCHK(hipGetLastError());
    }
    cover_finish_kernel<<<cdiv(L, 64), 64, 0, st>>>(d_r2, L, c->radius);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));   // the cover is complete; the sums may go
    return 0;
}

// The pruning pass of one call.  d_qs [nq][d] on the device, enqueued on h->stream; radius [nq] on the host.
struct CoverPass {
    lmi_index* h;
    const lmi_cover* c;
    CallScratch mem;
    const float* d_qs = nullptr;
    int nq = 0, W = 0;
    int64_t Q = 0, groups = 0;
    float* d_radius = nullptr;
    double* d_qn = nullptr;
    unsigned* d_bitmap = nullptr;
    int* d_counts = nullptr;
    std::vector<int32_t> counts;   // [nq], on the host once count() has returned
    int32_t max_count = 0;
    int64_t admitted = 0;

    CoverPass(lmi_index* h_, const lmi_cover* c_, const char* who) : h(h_), c(c_), mem(who) {}

    int open(const float* d_qs_, int nq_, const float* radius) {
        namespace cp = lmi_cover_plan;
        d_qs = d_qs_;
        nq = nq_;
        W = (int)cp::words_per_query(c->L);
        Q = cp::query_rows_for(g_cover_query_rows, nq, c->L);
        groups = cp::groups_for(nq, Q);
        CHK(mem.alloc(&d_radius, (size_t)nq * 4, "radius"));
        CHK(mem.alloc(&d_qn, (size_t)nq * 8, "query norms"));
        CHK(mem.alloc(&d_bitmap, (size_t)Q * W * 4, "admission bitmap"));
        CHK(mem.alloc(&d_counts, (size_t)nq * 4, "counts"));
        HIPCHK(hipMemcpyAsync(d_radius, radius, (size_t)nq * 4, hipMemcpyHostToDevice, h->stream));
        cover_qnorm_kernel<<<cdiv(nq, 256), 256, 0, h->stream>>>(d_qs, nq, c->d, d_qn);
        HIPCHK(hipGetLastError());
        return 0;
    }
    int64_t first(int64_t g) const { return g * Q; }
    int rows(int64_t g) const { return (int)std::min<int64_t>(Q, nq - g * Q); }
    // group g's verdicts into the bitmap
    int admit(int64_t g) {
        const int64_t q0 = first(g);
        const int gq = rows(g);
        const dim3 grid((unsigned)cdiv(gq, COVER_Q_PER_BLOCK), (unsigned)(W / 2));
        cover_admit_kernel<<<grid, 256, 0, h->stream>>>(c->metric, d_qs + (size_t)q0 * c->d, d_qn + q0, d_radius + q0, gq, c->d, c->centres, c->cn,
                                                       c->radius, c->d_nb_rows, c->L, W, d_bitmap);
        HIPCHK(hipGetLastError());
        return 0;
    }
    // every group judged and counted; the counts on the host (the pass's one synchronisation)
    int count() {
        for (int64_t g = 0; g < groups; ++g) {
            CHK(admit(g));
            cover_compact_kernel<<<rows(g), 64, 0, h->stream>>>(d_bitmap, W, 0, nullptr, d_counts + first(g));
            HIPCHK(hipGetLastError());
        }
        counts.assign((size_t)nq, 0);
        HIPCHK(hipMemcpyAsync(counts.data(), d_counts, (size_t)nq * 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        (void)lmi_cover_plan::first_over(counts.data(), nq, INT32_MAX, &max_count);
        admitted = 0;
        for (int32_t v : counts) admitted += v;
        return 0;
    }
    // the order, [nq][nb] on the device; nb >= max_count.  One group: its bitmap still stands.
    int write(int* d_order, int nb) {
        for (int64_t g = 0; g < groups; ++g) {
            if (groups > 1) CHK(admit(g));
            cover_compact_kernel<<<rows(g), 64, 0, h->stream>>>(d_bitmap, W, nb, d_order + (size_t)first(g) * nb, d_counts + first(g));
            HIPCHK(hipGetLastError());
        }
        return 0;
    }
    void report(int nb_used) const {
        g_cover_last[LMI_COVER_PLAN_GROUPS] = groups;
        g_cover_last[LMI_COVER_PLAN_QUERY_ROWS] = Q;
        g_cover_last[LMI_COVER_PLAN_BUCKETS] = c->L;
        g_cover_last[LMI_COVER_PLAN_ADMITTED] = admitted;
        g_cover_last[LMI_COVER_PLAN_MAX_PER_QUERY] = max_count;
        g_cover_last[LMI_COVER_PLAN_NB_USED] = nb_used;
        g_cover_last[LMI_COVER_PLAN_WORKSPACE_BYTES] = mem.total;
    }
};

// the pass's counts to the caller's array (nullable), a host or a device pointer; enqueued, not synchronised
int cover_counts_out(lmi_index* h, const CoverPass& P, int32_t* counts, int on_device) {
    if (!counts) return 0;
    if (on_device) HIPCHK(hipMemcpyAsync(counts, P.d_counts, (size_t)P.nq * 4, hipMemcpyDeviceToDevice, h->stream));
    else std::copy(P.counts.begin(), P.counts.end(), counts);
    return 0;
}

int cover_order_impl(lmi_index* h, const lmi_cover* c, const char* who, const float* queries_search, int nq, const float* radius, int nb,
                     int32_t* bucket_order, int32_t* counts, int on_device) {
    const void* qs = nullptr;
    CHK(input_ptr(h, queries_search, (size_t)nq * h->d_user * 4, on_device, h->q_srch, &qs));
    CoverPass P(h, c, who);
    CHK(P.open(static_cast<const float*>(qs), nq, radius));
    CHK(P.count());
    if (bucket_order) {
        int32_t unused = 0;
        const int64_t bad = lmi_cover_plan::first_over(P.counts.data(), nq, nb, &unused);
        if (bad >= 0)
            return fail("%s: query %lld admits %d buckets, more than nb = %d; nothing was written (count first with a NULL bucket_order)", who,
                        (long long)bad, (int)P.counts[(size_t)bad], nb);
        const size_t bytes = (size_t)nq * nb * 4;
        int* d_order = bucket_order;
        if (!on_device) {
            CHK(h->order.reserve(bytes));
            d_order = h->order.as<int>();
        }
        CHK(P.write(d_order, nb));
        if (!on_device) HIPCHK(hipMemcpyAsync(bucket_order, d_order, bytes, hipMemcpyDeviceToHost, h->stream));
    }
    CHK(cover_counts_out(h, P, counts, on_device));
    HIPCHK(hipStreamSynchronize(h->stream));   // the outputs have landed; the pass's buffers may go
    P.report(bucket_order ? nb : 0);
    return 0;
}

int range_exact_impl(lmi_index* h, const lmi_cover* c, const char* who, const float* queries_search, int nq, const float* radius,
                     const lmi_filter* f, const int32_t* filter_of, int64_t max_total, lmi_range_result** result, int32_t* nb_used,
                     int32_t* counts, int on_device) {
    const void* qs = nullptr;
    CHK(input_ptr(h, queries_search, (size_t)nq * h->d_user * 4, on_device, h->q_srch, &qs));
    begin_call(h);
    CoverPass P(h, c, who);
    CHK(P.open(static_cast<const float*>(qs), nq, radius));
    CHK(P.count());
    if (P.max_count > lmi_cover_plan::MAX_ORDER_BUCKETS) {
        int32_t unused = 0;
        const int64_t bad = lmi_cover_plan::first_over(P.counts.data(), nq, lmi_cover_plan::MAX_ORDER_BUCKETS, &unused);
        return fail("%s: query %lld needs %d buckets, more than the %d one range scan visits (splitting a query into several scans is not "
                    "offered); no result was made",
                    who, (long long)bad, (int)P.counts[(size_t)bad], lmi_cover_plan::MAX_ORDER_BUCKETS);
    }
    const int nb = std::max<int>(1, P.max_count);
    CHK(union_check(h, who, nq, nb, 1));   // what the scan refuses of this nb
    CHK(h->order.reserve((size_t)nq * nb * 4));
    CHK(P.write(h->order.as<int>(), nb));
    CHK(range_core(h, who, static_cast<const float*>(qs), nq, h->order.as<int>(), nb, radius, f, filter_of, max_total, result));
    if (cover_counts_out(h, P, counts, on_device) != 0 || hipStreamSynchronize(h->stream) != hipSuccess) {
        delete *result;
        *result = nullptr;
        return fail("%s: the counts could not be copied out", who);
    }
    if (nb_used) *nb_used = nb;
    P.report(nb);
    return 0;
}

}  // namespace

extern "C" LMI_API int lmi_cover_create(lmi_index* h, lmi_cover** out) {
    const char* who = "lmi_cover_create";
    if (!out) return fail("%s: out is NULL", who);
    *out = nullptr;
    if (!h) return fail("%s: NULL handle", who);
    if (h->building || !h->built) return fail("%s: the bucket index is not built (lmi_buckets_end has not run)", who);
    CHK(rowmajor_check(h, who));
    if (h->L > 65535) return fail("%s: an index of %d buckets (more than 65535) is not supported", who, h->L);
    for (int b = 0; b < h->L; ++b)
        if (h->h_nb_rows[b] > lmi_cover_plan::MAX_BUCKET_ROWS)
            return fail("%s: bucket %d holds %d rows, more than 2^26: the int64 sums of its centre could overflow", who, b, h->h_nb_rows[b]);
    CHK(set_dev(h));
    HIPCHK(hipStreamSynchronize(h->stream));   // what was enqueued on h before the call (a build's tail, a mutation) is in the slabs
    lmi_cover* c = new lmi_cover();
    c->stamp = h->layout_stamp;
    c->device = h->device;
    c->L = h->L;
    c->d = h->d_user;
    c->metric = h->metric;
    c->nb_rows = h->h_nb_rows;
    int rc;
    {
        CallScratch mem(who);
        rc = cover_fill(h, c, mem);
        if (rc != 0) (void)hipStreamSynchronize(h->stream);   // no kernel may still write what is about to be freed
    }
    if (rc != 0) {
        delete c;
        return -1;
    }
    *out = c;
    return 0;
}

extern "C" LMI_API int lmi_cover_destroy(lmi_cover* c) {
    if (!c) return 0;
    (void)hipSetDevice(c->device);
    delete c;   // (every call that reads a cover returns when its outputs have landed: nothing in flight reads it)
    return 0;
}

extern "C" LMI_API int lmi_cover_read(const lmi_cover* c, float* centres, float* radius, int64_t* counts) {
    if (!c) return fail("lmi_cover_read: NULL cover");
    HIPCHK(hipSetDevice(c->device));
    if (centres) HIPCHK(hipMemcpy(centres, c->centres, (size_t)c->L * c->d * 4, hipMemcpyDeviceToHost));
    if (radius) HIPCHK(hipMemcpy(radius, c->radius, (size_t)c->L * 4, hipMemcpyDeviceToHost));
    if (counts)
        for (int b = 0; b < c->L; ++b) counts[b] = c->nb_rows[(size_t)b];
    return 0;
}

extern "C" LMI_API int lmi_cover_order(lmi_index* h, const lmi_cover* c, const float* queries_search, int nq, const float* radius, int nb,
                                       int32_t* bucket_order, int32_t* counts, int on_device) {
    const char* who = "lmi_cover_order";
    for (int64_t& w : g_cover_last) w = 0;
    if (!h) return fail("%s: NULL handle", who);
    if (!h->built) return fail("%s: the bucket index is not built (lmi_buckets_begin/add_rows/end)", who);
    CHK(rowmajor_check(h, who));
    CHK(cover_check(h, who, c));
    if (nq < 0) return fail("%s: nq %d is negative", who, nq);
    if (bucket_order && nb < 1) return fail("%s: nb %d must be at least 1 where an order is asked for", who, nb);
    if (bucket_order && (long long)nq * nb >= (1ll << 31)) return fail("%s: nq*nb too large", who);
    if (nq == 0) return 0;
    if (!queries_search || !radius) return fail("%s: queries_search and radius must not be NULL", who);
    CHK(set_dev(h));
    if (cover_order_impl(h, c, who, queries_search, nq, radius, nb, bucket_order, counts, on_device) != 0) {
        (void)hipStreamSynchronize(h->stream);   // no kernel may still use the pass's buffers, which have freed themselves
        return -1;
    }
    return 0;
}

extern "C" LMI_API int lmi_search_range_exact(lmi_index* h, const lmi_cover* c, const float* queries_search, int nq, const float* radius,
                                              const lmi_filter* f, const int32_t* filter_of, int64_t max_total, lmi_range_result** result,
                                              int32_t* nb_used, int32_t* counts, int on_device) {
    const char* who = "lmi_search_range_exact";
    for (int64_t& w : g_cover_last) w = 0;
    CHK(range_begin(h, who, nq, 1, radius, f, filter_of, max_total, result));
    CHK(cover_check(h, who, c));
    if (nq == 0) {
        if (nb_used) *nb_used = 1;
        return range_empty(h, 0, 1, result);
    }
    if (!queries_search) return fail("%s: queries_search must not be NULL", who);
    CHK(set_dev(h));
    if (range_exact_impl(h, c, who, queries_search, nq, radius, f, filter_of, max_total, result, nb_used, counts, on_device) != 0) {
        (void)hipStreamSynchronize(h->stream);
        return -1;
    }
    return 0;
}

extern "C" LMI_API int lmi_cover_set_geometry(int64_t query_rows) {
    if (!lmi_cover_plan::query_rows_ok(query_rows))
        return fail("lmi_cover_set_geometry: query_rows %lld outside [0, 2^20]", (long long)query_rows);
    g_cover_query_rows = query_rows;
    return 0;
}

extern "C" LMI_API int lmi_debug_cover_plan(int64_t* out, int n) {
    if (!out || n < 0) return fail("lmi_debug_cover_plan: NULL argument");
    for (int i = 0; i < std::min(n, (int)LMI_COVER_PLAN_COUNT); ++i) out[i] = g_cover_last[i];
    return 0;
}
