// lmi_host_regroup.h -- lmi_regroup: a second, independent index that holds a built index's objects under new bucket labels, the
// geometry hook and the plan words (kernels: lmi_regroup.h; the arithmetic: lmi_regroup_plan.h; include/lmi_hip.h states the contract).
#pragma once
#include "lmi_host_call.h"
#include "lmi_host_subset.h"
#include "lmi_regroup.h"
#include "lmi_regroup_plan.h"

// ------------------------------------------------------------------------------------------------
// No reference counterpart (the reference re-labels its DataFrames and rebuilds).  lmi_subset is "same labels, fewer objects"; this is
// "same objects, new labels, any new L".  The new handle is what lmi_create + the source's settings + lmi_buckets_begin(L_new, new
// labels) / add_rows / end over "the source's objects in the order it holds them" would be: every row gets its label and its word on
// the device, the words are sorted (so a new bucket's objects are in (old bucket, old row) order whatever the list's or the map's order
// is), the host lays the new index out from the counts per new label (begin_layout), lmi_subset's gathers move the stored images, and
// what a build derives from the rows is derived from the new handle's own rows.  The source is only read.
// The call's maps, per object of the source: 8 + 8 bytes (the words and the merge passes' second buffer; 8 when one tile holds them
// all) + 4 (the slab row of its ordinal); per slab row of the new index: 4 (the gathers' source position); per list entry: 8 (its id
// and its label).  All of them are freed before the call returns (lmi_regroup_plan.h: SortPlan::map_bytes).
namespace {
thread_local int64_t g_regroup_tile_rows = 0;   // 0: lmi_regroup_plan::DEFAULT_TILE_ROWS
thread_local int64_t g_regroup_last[LMI_REGROUP_PLAN_COUNT] = {};
}  // namespace

// everything of lmi_regroup behind the argument checks: fills the fresh handle c from h (h->stream is idle; c runs on the NULL stream)
static int regroup_fill(lmi_index* h, lmi_index* c, const lmi_regroup_plan::List& list, const std::vector<int>& map, int L_new, int64_t* n_named) {
    namespace rp = lmi_regroup_plan;
    const int L = h->L;
    hipStream_t st = c->stream;
    // ---- h's settings and copies of all its models; not the tree, whose child_bucket entries name h's buckets ----
    CHK(inherit_handle(h, c, false));
    // ---- 1: every row's new label, its word and its slab row at its ordinal; the counts come back to the host ----
    const std::vector<int64_t> base64 = rp::ordinal_bases(h->h_nb_rows);
    const int64_t n = base64[L];
    const rp::SortPlan P = rp::sort_plan(n, g_regroup_tile_rows);
    std::vector<int> base(base64.begin(), base64.end() - 1);   // (n < 2^31: begin_checks of the build that made h)
    CallScratch mem("lmi_regroup");
    unsigned long long *kA = nullptr, *kB = nullptr, *d_counters = nullptr;
    int *ord_row = nullptr, *d_map = nullptr, *d_base = nullptr, *d_list_label = nullptr, *d_first = nullptr, *srcpos = nullptr;
    uint32_t* d_list = nullptr;
    const size_t n_list = list.ids.size();
    const size_t counter_bytes = 8 + ((size_t)L_new + L) * 4 + 16;   // named | counts [L_new] | left [L] | the fp16 gather's maximum
    std::vector<unsigned char> counters(counter_bytes, 0);
    CHK(mem.alloc(&d_counters, counter_bytes, "counters"));
    if (n > 0) {
        CHK(mem.alloc(&kA, (size_t)n * 8, "words"));
        if (P.passes > 0) CHK(mem.alloc(&kB, (size_t)n * 8, "second word buffer"));
        CHK(mem.alloc(&ord_row, (size_t)n * 4, "slab rows by ordinal"));
        CHK(mem.alloc(&d_map, (size_t)L * 4, "bucket map"));
        CHK(mem.alloc(&d_base, (size_t)L * 4, "ordinal bases"));
        CHK(mem.alloc(&d_list, std::max<size_t>(n_list, 1) * 4, "listed ids"));
        CHK(mem.alloc(&d_list_label, std::max<size_t>(n_list, 1) * 4, "listed labels"));
        CHK(mem.alloc(&d_first, (size_t)L_new * 4, "first rows of the new labels"));
    }
    int* d_counts = reinterpret_cast<int*>(d_counters + 1);
    int* d_left = d_counts + L_new;
    unsigned* d_maxbits = reinterpret_cast<unsigned*>(d_left + L);
    HIPCHK(hipMemsetAsync(d_counters, 0, counter_bytes, st));
    if (n > 0) {
        HIPCHK(hipMemcpyAsync(d_map, map.data(), (size_t)L * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_base, base.data(), (size_t)L * 4, hipMemcpyHostToDevice, st));
        if (n_list) {
            HIPCHK(hipMemcpyAsync(d_list, list.ids.data(), n_list * 4, hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync(d_list_label, list.labels.data(), n_list * 4, hipMemcpyHostToDevice, st));
        }
        const int max_n = *std::max_element(h->h_nb_rows.begin(), h->h_nb_rows.end());
        regroup_label_kernel<<<dim3(std::max(1, std::min(64, cdiv(max_n, 256))), L), 256, 0, st>>>(
            h->ids_slab.as<uint32_t>(), h->d_rb_start.as<int>(), h->d_nb_rows.as<int>(), d_base, d_list, d_list_label, (int)n_list, d_map, kA,
            ord_row, d_counts, d_left, d_counters);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(counters.data(), d_counters, counter_bytes, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    unsigned long long named = 0;
    memcpy(&named, counters.data(), 8);
    const int* h_counts = reinterpret_cast<const int*>(counters.data() + 8);
    const std::vector<int> left(h_counts + L_new, h_counts + L_new + L);
    if (const int b = rp::first_unmapped(left); b >= 0)
        return fail("bucket %d maps to -1 (it must be emptied by the list), but %d of its %d objects are not in the list", b, left[(size_t)b],
                    h->h_nb_rows[(size_t)b]);
    // ---- 2: the layout of a fresh build under the new labels ----
    std::vector<int> cnt(h_counts, h_counts + L_new), first((size_t)L_new, 0);
    std::vector<unsigned char> any((size_t)L_new, 0);
    int64_t sum = 0;
    for (int b = 0; b < L_new; ++b) {
        first[(size_t)b] = (int)sum;
        sum += cnt[(size_t)b];
        any[(size_t)b] = cnt[(size_t)b] > 0;
    }
    if (sum != n) return fail("internal: %lld of %lld objects were labelled (%s:%d)", (long long)sum, (long long)n, __FILE__, __LINE__);
    CHK(begin_layout(c, n, h->d_user, L_new, cnt.data(), any.data(), nullptr, "lmi_regroup"));
    if (c->d != h->d || c->dp != h->dp || c->KGs != h->KGs || (c->prefilter && c->storage == LMI_STORAGE_F16 && (c->KG16 != h->KG16 || frag16x16(c) != frag16x16(h))))
        return fail("internal: the new handle's images are shaped differently from the source's (%s:%d)", __FILE__, __LINE__);
    const int64_t new_rows = c->n_rb_total * 32;
    HIPCHK(hipMemsetAsync(c->ids_slab.p, 0, (size_t)std::max<int64_t>(c->n_rb_total, 1) * 32 * 4, st));
    if (n > 0) {
        // ---- 3: the words in ascending order: tiles in LDS, then runs doubled until one holds them all ----
        const int T = (int)P.tile_rows, M = (int)P.merge_rows;
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&regroup_runs_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)(rp::MAX_TILE_ROWS * 8)));
        regroup_runs_kernel<<<(unsigned)P.tiles, RANGE_SORT_BLOCK, (size_t)T * 8, st>>>(kA, n, T);
        HIPCHK(hipGetLastError());
        unsigned long long *src = kA, *dst = kB;
        for (int64_t run = T; run < n; run <<= 1) {
            range_sort_merge_kernel<<<(unsigned)P.merge_pieces, RANGE_SORT_BLOCK, (size_t)M * 8, st>>>(src, n, run, M, dst);
            HIPCHK(hipGetLastError());
            std::swap(src, dst);
        }
        // ---- 4: per row of the NEW slab the slab row of h it comes from (-1 behind a bucket's last row), then the gather of the
        //         stored image with the ids alongside (lmi_subset.h's kernels) ----
        CHK(mem.alloc(&srcpos, (size_t)new_rows * 4, "source positions"));
        HIPCHK(hipMemsetAsync(srcpos, 0xFF, (size_t)new_rows * 4, st));
        HIPCHK(hipMemcpyAsync(d_first, first.data(), (size_t)L_new * 4, hipMemcpyHostToDevice, st));
        regroup_srcpos_kernel<<<gather_blocks(c, n), 256, 0, st>>>(src, n, ord_row, d_first, c->d_rb_start.as<int>(), srcpos);
        HIPCHK(hipGetLastError());
        switch (stored_form(c)) {
        case FORM_FRAG16: {
            const long long pieces = c->n_rb_total * c->KG16 * 64;
            subset_gather_frag16_kernel<<<gather_blocks(c, pieces), 256, 0, st>>>(h->slab16.as<uint4>(), h->ids_slab.as<uint32_t>(), srcpos, c->n_rb_total,
                                                                                   c->KG16, frag16x16(c), c->slab16.as<uint4>(), c->ids_slab.as<uint32_t>(),
                                                                                   d_maxbits);
            break;
        }
        case FORM_ROWMAJOR: {
            const long long pieces = new_rows * (c->dp / 4);
            subset_gather_rows_kernel<<<gather_blocks(c, pieces), 256, 0, st>>>(h->rowmajor.as<float4>(), h->ids_slab.as<uint32_t>(), srcpos, new_rows,
                                                                                 c->dp / 4, c->rowmajor.as<float4>(), c->ids_slab.as<uint32_t>());
            break;
        }
        case FORM_FRAG32: {
            const long long pieces = c->n_rb_total * c->KGs * 64;
            subset_gather_frag32_kernel<<<gather_blocks(c, pieces), 256, 0, st>>>(h->slab.as<float4>(), h->ids_slab.as<uint32_t>(), srcpos, c->n_rb_total,
                                                                                   c->KGs, c->slab.as<float4>(), c->ids_slab.as<uint32_t>());
            break;
        }
        }
        HIPCHK(hipGetLastError());
    }
    // ---- 5: what lmi_buckets_end derives from the rows, from the new handle's own ----
    c->rows_added = c->N;
    c->have16 = false;
    if (stored_form(c) == FORM_FRAG16 && c->n_rb_total > 0) {
        // the object set is h's, so the absmax and the scale are h's and the halves are right as they were moved; only the buckets'
        // norm maxima belong to the new partition
        CHK(reset_norm_tables(c));
        HIPCHK(hipMemcpyAsync(c->xscale.p, h->xscale.p, 8, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipMemcpyAsync(c->xmaxbits.p, h->xmaxbits.p, 16, hipMemcpyDeviceToDevice, st));
        bucket_norm16_kernel<<<dim3(64, c->L), 256, 0, st>>>(c->slab16.as<uint4>(), c->d, c->KG16, frag16x16(c), c->d_rb_start.as<int>(),
                                                            c->d_nb_rows.as<int>(), c->bnorm.as<unsigned>());
        HIPCHK(hipGetLastError());
        c->have16 = true;
    } else if (c->prefilter && c->n_rb_total > 0) {
        CHK(prefilter_images(c));   // its own absmax, scale, fp16 fragments and norms
    }
    HIPCHK(hipStreamSynchronize(st));   // (the maps free themselves behind it)
    c->building = false;
    c->built = true;
    c->layout_stamp = next_layout_stamp();   // its own layout: no filter of the source fits it
    if (n_named) *n_named = (int64_t)named;
    g_regroup_last[LMI_REGROUP_PLAN_ROWS] = n;
    g_regroup_last[LMI_REGROUP_PLAN_TILE_ROWS] = P.tile_rows;
    g_regroup_last[LMI_REGROUP_PLAN_TILES] = P.tiles;
    g_regroup_last[LMI_REGROUP_PLAN_MERGE_ROWS] = P.merge_rows;
    g_regroup_last[LMI_REGROUP_PLAN_PASSES] = P.passes;
    g_regroup_last[LMI_REGROUP_PLAN_MAP_BYTES] = mem.total;
    g_regroup_last[LMI_REGROUP_PLAN_NAMED] = (int64_t)named;
    return 0;
}

extern "C" LMI_API int lmi_regroup_set_geometry(int64_t tile_rows) {
    namespace rp = lmi_regroup_plan;
    if (!rp::tile_rows_ok(tile_rows))
        return fail("lmi_regroup_set_geometry: tile_rows %lld is not 0 or a power of two in [%lld, %lld]", (long long)tile_rows,
                    (long long)rp::MIN_TILE_ROWS, (long long)rp::MAX_TILE_ROWS);
    g_regroup_tile_rows = tile_rows;
    return 0;
}

extern "C" LMI_API int lmi_debug_regroup_plan(int64_t* out, int n) {
    if (!out || n < 0) return fail("lmi_debug_regroup_plan: NULL argument");
    for (int i = 0; i < std::min(n, (int)LMI_REGROUP_PLAN_COUNT); ++i) out[i] = g_regroup_last[i];
    return 0;
}

extern "C" LMI_API int lmi_regroup(lmi_index* h, const uint32_t* ids, const int64_t* labels, int64_t n, const int32_t* bucket_map, int L_new,
                                   lmi_index** out, int64_t* n_named) {
    namespace rp = lmi_regroup_plan;
    for (int64_t& w : g_regroup_last) w = 0;
    if (!out) return fail("lmi_regroup: out is NULL");
    *out = nullptr;
    if (n_named) *n_named = 0;
    if (!h) return fail("lmi_regroup: NULL handle");
    if (h->building) return fail("lmi_regroup: the index is being built (lmi_buckets_end has not run)");
    if (!h->built) return fail("lmi_regroup: the bucket index is not built (lmi_buckets_end has not run)");
    if (!h->h_owned.empty())
        return fail("lmi_regroup: the index was built with an `owned` mask (a sharded rank): a new partition needs a new ownership, which "
                    "this call does not take");
    rp::List list;
    const rp::Verdict v = rp::check(h->L, L_new, ids, labels, n, bucket_map, list);
    switch (v.problem) {
    case rp::OK: break;
    case rp::BAD_L_NEW: return fail("lmi_regroup: L_new = %lld outside [1, %lld)", (long long)v.value, (long long)rp::MAX_LABELS);
    case rp::BAD_N: return fail("lmi_regroup: bad arguments (n = %lld is negative)", (long long)v.value);
    case rp::NULL_LIST: return fail("lmi_regroup: bad arguments (ids and labels are required when n > 0)");
    case rp::BAD_LABEL: return fail("lmi_regroup: labels[%lld] = %lld outside [0,%d)", (long long)v.at, (long long)v.value, L_new);
    case rp::BAD_MAP: return fail("lmi_regroup: bucket_map[%lld] = %lld outside [-1,%d)", (long long)v.at, (long long)v.value, L_new);
    case rp::NULL_MAP_SHRINKS:
        return fail("lmi_regroup: a NULL bucket_map is the identity and needs L_new >= L (L_new = %d, L = %d)", L_new, h->L);
    case rp::DUPLICATE_ID: return fail("lmi_regroup: id %u is listed twice", (unsigned)v.value);
    }
    CHK(set_dev(h));
    HIPCHK(hipStreamSynchronize(h->stream));   // what was enqueued on h before the call (a build's tail, a mutation) is in the slabs
    lmi_index* c = nullptr;
    if (lmi_create(h->device, &c) != 0) return fail("lmi_regroup: %s", std::string(g_err).c_str());
    if (regroup_fill(h, c, list, rp::map_of(h->L, bucket_map), L_new, n_named) != 0) {   // the new handle and everything the call allocated go
        const std::string why = g_err;
        (void)hipStreamSynchronize(c->stream);
        (void)lmi_destroy(c);
        if (n_named) *n_named = 0;
        return fail("lmi_regroup: %s; no index was made and the source is unchanged", why.c_str());
    }
    *out = c;
    return 0;
}
