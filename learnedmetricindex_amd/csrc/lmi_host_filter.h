// lmi_host_filter.h -- filter sets over a built index (kernels: lmi_filter.h; the lists' arithmetic: lmi_filter_plan.h):
// lmi_filter_create / _destroy / _counts / _bucket_mask, lmi_debug_filter_plan, and what lmi_host_union.h asks of a filter before a
// filtered union call (filter_check).  No reference counterpart (the reference filters its DataFrames and rebuilds).
#pragma once
#include "lmi_host.h"
#include "lmi_host_call.h"
#include "lmi_filter.h"
#include "lmi_filter_plan.h"

static_assert(LMI_FILTER_KEEP == lmi_filter_plan::KEEP && LMI_FILTER_DROP == lmi_filter_plan::DROP && LMI_FILTER_MAX == lmi_filter_plan::MAX_FILTERS,
              "lmi_filter_plan.h restates the modes and the limit of a filter set");

// A filter set: the masks on the device, keyed by slab position, and what the host needs of the layout they were made under.  It holds
// no pointer to the handle: the stamp says which handles it fits.
struct lmi_filter {
    uint64_t stamp = 0;              // the layout stamp of the handle it was made from
    int device = 0, nf = 0, L = 0;
    int64_t n_rb_total = 0;
    std::vector<int> nb_rows, rb_start;   // the layout: rows and first row-block per bucket
    std::vector<int32_t> counts;          // [nf][L]: the allowed rows
    DevBuf mask;                          // [nf][n_rb_total] words
    int64_t mask_bytes() const { return (int64_t)nf * n_rb_total * 4; }
};

namespace {

thread_local int64_t g_filter_last[LMI_FILTER_PLAN_COUNT] = {};

// what a filtered union call refuses beyond union_check, before any launch
int filter_check(const lmi_index* h, const char* who, const lmi_filter* f, const int32_t* filter_of, int64_t nq) {
    if (!f) return fail("%s: NULL filter", who);
    if (f->stamp != h->layout_stamp || f->device != h->device)
        return fail("%s: the filter is stale or belongs to another index: it was made under layout stamp %llu, this handle carries %llu "
                    "(lmi_buckets_insert / _delete and lmi_subset give a new layout; make the filter again)",
                    who, (unsigned long long)f->stamp, (unsigned long long)h->layout_stamp);
    const int64_t bad = lmi_filter_plan::first_bad_filter_of(filter_of, nq, f->nf);
    if (bad >= 0) return fail("%s: filter_of[%lld] = %d outside [-1,%d)", who, (long long)bad, (int)filter_of[bad], f->nf);
    return 0;
}

int filter_fill(lmi_index* h, lmi_filter* f, const lmi_filter_plan::Lists& lists, const int32_t* modes) {
    const int L = h->L, nf = f->nf;
    hipStream_t st = h->stream;
    CHK(f->mask.reserve((size_t)std::max<int64_t>(f->mask_bytes(), 4)));
    HIPCHK(hipMemsetAsync(f->mask.p, 0, (size_t)std::max<int64_t>(f->mask_bytes(), 4), st));
    const int max_n = L > 0 ? *std::max_element(f->nb_rows.begin(), f->nb_rows.end()) : 0;
    if (max_n > 0) {
        CallScratch mem("lmi_filter_create");
        uint32_t* d_list = nullptr;
        int *d_off = nullptr, *d_modes = nullptr, *d_counts = nullptr;
        CHK(mem.alloc(&d_list, lists.ids.size() * 4, "id lists"));
        CHK(mem.alloc(&d_off, (size_t)(nf + 1) * 4, "list offsets"));
        CHK(mem.alloc(&d_modes, (size_t)nf * 4, "modes"));
        CHK(mem.alloc(&d_counts, (size_t)nf * L * 4, "counts"));
        if (!lists.ids.empty()) HIPCHK(hipMemcpyAsync(d_list, lists.ids.data(), lists.ids.size() * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_off, lists.off.data(), (size_t)(nf + 1) * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_modes, modes, (size_t)nf * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemsetAsync(d_counts, 0, (size_t)nf * L * 4, st));
        filter_mark_kernel<<<dim3(cdiv(max_n, 256), L, nf), 256, 0, st>>>(h->ids_slab.as<uint32_t>(), h->d_rb_start.as<int>(), h->d_nb_rows.as<int>(), d_list,
                                                                          d_off, d_modes, (long long)f->n_rb_total, L, f->mask.as<unsigned>(), d_counts);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(f->counts.data(), d_counts, (size_t)nf * L * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));   // the lists, the counts and the call's allocations may go
    }
    return 0;
}

}  // namespace

extern "C" LMI_API int lmi_filter_create(lmi_index* h, const uint32_t* ids, const int64_t* offsets, int nf, const int32_t* modes, lmi_filter** out) {
    const char* who = "lmi_filter_create";
    if (!out) return fail("%s: out is NULL", who);
    *out = nullptr;
    if (!h) return fail("%s: NULL handle", who);
    if (h->building || !h->built) return fail("%s: the bucket index is not built (lmi_buckets_end has not run)", who);
    int bad = -1;
    if (const char* why = lmi_filter_plan::check_lists(ids, offsets, nf, modes, &bad)) {
        if (bad >= 0) return fail("%s: %s (filter %d: mode %d, ids [%lld, %lld))", who, why, bad, (int)modes[bad], (long long)offsets[bad], (long long)offsets[bad + 1]);
        return fail("%s: %s (nf = %d)", who, why, nf);
    }
    if (h->L > 65535) return fail("%s: an index of %d buckets (more than 65535) is not supported", who, h->L);
    CHK(set_dev(h));
    HIPCHK(hipStreamSynchronize(h->stream));   // what was enqueued on h before the call (a build's tail, a mutation) is in the slabs
    const lmi_filter_plan::Lists lists = lmi_filter_plan::normalise(ids, offsets, nf);
    lmi_filter* f = new lmi_filter();
    f->stamp = h->layout_stamp;
    f->device = h->device;
    f->nf = nf;
    f->L = h->L;
    f->n_rb_total = h->n_rb_total;
    f->nb_rows = h->h_nb_rows;
    f->rb_start.assign(h->h_rb_start.begin(), h->h_rb_start.begin() + h->L);
    f->counts.assign((size_t)nf * h->L, 0);
    if (filter_fill(h, f, lists, modes) != 0) {
        (void)hipStreamSynchronize(h->stream);
        delete f;
        return -1;
    }
    *out = f;
    return 0;
}

extern "C" LMI_API int lmi_filter_destroy(lmi_filter* f) {
    if (!f) return 0;
    (void)hipSetDevice(f->device);
    delete f;   // (a filtered call returns when its outputs have landed: nothing in flight reads the masks)
    return 0;
}

extern "C" LMI_API int lmi_filter_counts(lmi_filter* f, int64_t* out) {
    if (!f || !out) return fail("lmi_filter_counts: NULL argument");
    for (size_t i = 0; i < f->counts.size(); ++i) out[i] = f->counts[i];
    return 0;
}

extern "C" LMI_API int lmi_filter_bucket_mask(lmi_filter* f, int j, int bucket, uint8_t* out) {
    if (!f) return fail("lmi_filter_bucket_mask: NULL filter");
    if (j < 0 || j >= f->nf) return fail("lmi_filter_bucket_mask: filter %d outside [0,%d)", j, f->nf);
    if (bucket < 0 || bucket >= f->L) return fail("lmi_filter_bucket_mask: bucket %d outside [0,%d)", bucket, f->L);
    const int n = f->nb_rows[bucket];
    if (n == 0) return 0;
    if (!out) return fail("lmi_filter_bucket_mask: out is NULL");
    HIPCHK(hipSetDevice(f->device));
    std::vector<unsigned> words((size_t)cdiv(n, 32));
    HIPCHK(hipMemcpy(words.data(), f->mask.as<unsigned>() + lmi_filter_plan::mask_word(j, f->n_rb_total, f->rb_start[bucket], 0), words.size() * 4,
                     hipMemcpyDeviceToHost));
    for (int r = 0; r < n; ++r) out[r] = (uint8_t)((words[(size_t)r >> 5] >> lmi_filter_plan::mask_bit(r)) & 1u);
    return 0;
}

extern "C" LMI_API int lmi_debug_filter_plan(int64_t* out, int n) {
    if (!out || n < 0) return fail("lmi_debug_filter_plan: NULL argument");
    for (int i = 0; i < std::min(n, (int)LMI_FILTER_PLAN_COUNT); ++i) out[i] = g_filter_last[i];
    return 0;
}
