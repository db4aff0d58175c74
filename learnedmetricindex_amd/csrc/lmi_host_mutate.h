// lmi_host_mutate.h -- lmi_buckets_insert / lmi_buckets_delete on a built index (kernels: lmi_mutate.h).
#pragma once
#include "lmi_host_build.h"

// ------------------------------------------------------------------------------------------------
// Mutation of a built index (no reference counterpart: the reference rebuilds).  Bucket b holds h_nb_rows[b] rows from
// row-block h_rb_start[b] on and has h_cap_rb[b] row-blocks reserved there; the slab's first n_rb_total row-blocks are
// buckets, their spare row-blocks and holes (the old places of relocated buckets), all of them zero where no row lives.
// An insert that overflows a bucket's capacity moves the bucket behind the last row-block with slack; when that does not
// fit the allocations, or the holes would pass a quarter of the slab, every bucket is re-packed into new allocations.
// A handle that is never mutated keeps lmi_buckets_end's layout byte for byte.  Where things go is decided in lmi_layout.h
// (plan_insert, delete_groups: pure host code, tested on the CPU); which images move is slab_images' table (lmi_host.h).
namespace {
int mut_check(lmi_index* h, const char* who) {
    if (!h) return fail("%s: NULL handle", who);
    if (!h->built) return fail("%s: the bucket index is not built (lmi_buckets_end has not run)", who);
    if (h->storage == LMI_STORAGE_F16)
        return fail("%s: an LMI_STORAGE_F16 index cannot be changed in place yet (mutation of a compact index is not implemented); rebuild it, or use LMI_STORAGE_F32", who);
    if (h->parent) return fail("%s: a clone view cannot change the index it borrows", who);
    if (h->live_clones > 0) return fail("%s: %d clone view(s) of this handle are alive (they hold copies of the bucket tables); destroy them first", who, h->live_clones);
    return 0;
}
bool owns(const lmi_index* h, int b) { return h->h_owned.empty() || h->h_owned[b]; }
}  // namespace

// N / owned_total / n_nonempty / chunk rows / h_nch from h_nb_rows, and the device copies of the bucket tables (on the stream)
static int mut_derive(lmi_index* h) {
    const int L = h->L;
    derive_tables(h, nullptr);   // (the chunk length stays the build's, unless a bucket has outgrown 1024 chunks of it)
    h->h_rb_start[L] = (int)h->n_rb_total;
    HIPCHK(hipMemcpyAsync(h->d_nb_rows.p, h->h_nb_rows.data(), L * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_rb_start.p, h->h_rb_start.data(), (L + 1) * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_nch.p, h->h_nch.data(), L * 4, hipMemcpyHostToDevice, h->stream));
    return 0;
}

// The rows of src marked against an id list, counted per bucket (lmi_buckets_delete; lmi_subset, whose new handle w marks the source's
// rows): the list sorted and deduplicated (one that arrives sorted is only checked), uploaded, w->mut_keep[slab row of src] <- the row
// stays (mode: LMI_SUBSET_KEEP / LMI_SUBSET_DROP), kept[L] <- the rows that stay per bucket, back on the host when the call returns.
// Runs on w's stream with w's maps (mut_ids, mut_keep, mut_word; mut_src and mut_list are reserved beside them); tail_bytes: zeroed words behind the counts in w->mut_word, for the caller.  Where no row can
// stay (src stores none, or nothing is listed to keep) nothing is reserved or launched.
static int mark_rows(lmi_index* src, lmi_index* w, const uint32_t* ids, int64_t n, int mode, size_t tail_bytes, std::vector<int>& kept) {
    const int L = src->L;
    kept.assign(L, 0);
    std::vector<uint32_t> list(ids, ids + n);
    if (!std::is_sorted(list.begin(), list.end())) std::sort(list.begin(), list.end());
    list.erase(std::unique(list.begin(), list.end()), list.end());
    if (src->owned_total == 0 || (mode == LMI_SUBSET_KEEP && list.empty())) return 0;
    CHK(w->mut_ids.reserve(std::max<size_t>(list.size(), 1) * 4));
    CHK(w->mut_keep.reserve((size_t)src->n_rb_total * 32 * 4));
    CHK(w->mut_src.reserve((size_t)src->n_rb_total * 32 * 4));   // (the caller's compaction map, compact_map_kernel: with the other maps, before the caller's images)
    CHK(w->mut_word.reserve((size_t)L * 4 + tail_bytes));
    CHK(w->mut_list.reserve((size_t)L * 4));   // (its bucket list; lmi_buckets_delete has reserved its longer lists)
    if (!list.empty()) HIPCHK(hipMemcpyAsync(w->mut_ids.p, list.data(), list.size() * 4, hipMemcpyHostToDevice, w->stream));
    HIPCHK(hipMemsetAsync(w->mut_word.p, 0, (size_t)L * 4 + tail_bytes, w->stream));
    const int max_n = *std::max_element(src->h_nb_rows.begin(), src->h_nb_rows.end());
    mark_rows_kernel<<<dim3(std::max(1, std::min(64, cdiv(max_n, 256))), L), 256, 0, w->stream>>>(
        src->ids_slab.as<uint32_t>(), src->d_rb_start.as<int>(), src->d_nb_rows.as<int>(), w->mut_ids.as<uint32_t>(), (int)list.size(), mode,
        w->mut_keep.as<int>(), w->mut_word.as<int>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(kept.data(), w->mut_word.p, (size_t)L * 4, hipMemcpyDeviceToHost, w->stream));
    HIPCHK(hipStreamSynchronize(w->stream));
    return 0;
}

// The fp16 images and the norm maxima of n row ranges a mutation touched, from their rows as they are now.  d_list (device): five
// lists of `stride` ints each, [bucket | first row | rows | first row-block | row-blocks] (range lists of lmi_mutate.h); conv_blocks:
// the conversion's blocks per range, max_rows: the longest range.
static int redo_ranges(lmi_index* h, const int* d_list, int stride, int n, int conv_blocks, int max_rows) {
    convert16_ranges_kernel<<<dim3(conv_blocks, n), 256, 0, h->stream>>>(h->rowmajor.as<float>(), h->d, h->dp, d_list + 3 * stride, d_list + 4 * stride,
                                                                        h->KG16, h->xscale.as<float>(), h->slab16.as<uint4>(), frag16x16(h));
    HIPCHK(hipGetLastError());
    bucket_norm_ranges_kernel<<<dim3(std::min(64, cdiv(max_rows, 256)), n), 256, 0, h->stream>>>(
        h->rowmajor.as<float>(), h->d, h->dp, d_list, d_list + stride, d_list + 2 * stride, h->xscale.as<float>(), h->bnorm.as<unsigned>(),
        h->bdelta.as<unsigned>());
    HIPCHK(hipGetLastError());
    return 0;
}

// Every bucket into new allocations of alloc_new row-blocks: bucket b's first nrb[b] row-blocks go from row-block from[b]
// to to[b].  Allocation failure frees what this call allocated and leaves the index as it was.
static int repack(lmi_index* h, const std::vector<int>& from, const std::vector<int>& to, const std::vector<int>& nrb, int64_t alloc_new) {
    SlabImage im[MAX_SLAB_IMAGES];
    const int n = slab_images(h, im);
    DevBuf fresh[MAX_SLAB_IMAGES];   // (an early return frees them)
    size_t bytes[MAX_SLAB_IMAGES] = {};
    for (int i = 0; i < n; ++i) {
        bytes[i] = im[i].bytes(alloc_new);
        hipError_t e = hipMalloc(&fresh[i].p, bytes[i]);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            fresh[i].p = nullptr;
            return fail("lmi_buckets_insert: growing the slab to %lld row-blocks failed (%s); the index is unchanged", (long long)alloc_new, hipGetErrorString(e));
        }
        fresh[i].cap = bytes[i];
    }
    for (int i = 0; i < n; ++i) HIPCHK(hipMemsetAsync(fresh[i].p, 0, bytes[i], h->stream));
    const int L = h->L;
    for (int b = 0; b < L;) {   // runs of buckets that are consecutive at both ends: one copy each (all of them after a build)
        int e = b + 1;
        int64_t len = nrb[b];
        while (e < L && from[e] == from[b] + len && to[e] == to[b] + len) len += nrb[e++];
        if (len > 0)
            for (int i = 0; i < n; ++i)
                HIPCHK(hipMemcpyAsync(fresh[i].as<char>() + (size_t)to[b] * im[i].rb_bytes, im[i].buf->as<char>() + (size_t)from[b] * im[i].rb_bytes,
                                      (size_t)len * im[i].rb_bytes, hipMemcpyDeviceToDevice, h->stream));
        b = e;
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int i = 0; i < n; ++i) *im[i].buf = std::move(fresh[i]);
    return 0;
}

// ---- insert, step by step ----
// 1 count: the rows every owned bucket receives (a label outside [0, L) refuses the call)
static int insert_count(lmi_index* h, const int64_t* labels, int64_t nrows, const char* who, std::vector<int64_t>& add, int64_t* stored) {
    const int L = h->L;
    add.assign(L, 0);
    *stored = 0;
    for (int64_t i = 0; i < nrows; ++i) {
        const int64_t b = labels[i];
        if (b < 0 || b >= L) return fail("%s: labels[%lld] = %lld outside [0,%d); nothing was inserted", who, (long long)i, (long long)b, L);
        if (owns(h, (int)b)) { add[b]++; ++*stored; }
    }
    return 0;
}

// 3 reserve: every allocation the call needs before the first change (a failure leaves the index as it was)
static int insert_reserve(lmi_index* h, int64_t nrows, int src16, int on_device) {
    CHK(ingest_piece_reserve(h, std::min(ingest_piece_rows(h), nrows), src16, false, on_device));
    CHK(h->mut_pos.reserve((size_t)nrows * 4));
    CHK(h->mut_ids.reserve((size_t)nrows * 4));
    CHK(h->mut_list.reserve((size_t)h->L * 5 * 4));
    CHK(h->mut_word.reserve(16));
    return 0;
}

// 4 move or re-pack: the planned layout becomes the handle's.  Without a re-pack a relocated bucket's old row-blocks go to the new
// place, zeros after them (past n_rb_total an allocation holds whatever it held), and zeros where they were (a hole: rescaling takes
// the absmax of every row-block of the layout)
static int insert_relocate(lmi_index* h, const lmi_layout::InsertPlan& p) {
    const int L = h->L;
    if (p.pack) {
        std::vector<int> from(h->h_rb_start.begin(), h->h_rb_start.begin() + L);
        CHK(repack(h, from, p.start, h->h_cap_rb, p.alloc_new));
    } else {
        SlabImage im[MAX_SLAB_IMAGES];
        const int nim = slab_images(h, im);
        for (int b = 0; b < L; ++b) {
            if (!p.moved[b]) continue;
            const int from = h->h_rb_start[b], nrb = h->h_cap_rb[b];
            for (int i = 0; i < nim; ++i) {
                char* base = im[i].buf->as<char>();
                const size_t rb = im[i].rb_bytes;
                if (nrb > 0) {
                    HIPCHK(hipMemcpyAsync(base + (size_t)p.start[b] * rb, base + (size_t)from * rb, (size_t)nrb * rb, hipMemcpyDeviceToDevice, h->stream));
                    HIPCHK(hipMemsetAsync(base + (size_t)from * rb, 0, (size_t)nrb * rb, h->stream));
                }
                HIPCHK(hipMemsetAsync(base + (size_t)(p.start[b] + nrb) * rb, 0, (size_t)(p.cap[b] - nrb) * rb, h->stream));
            }
        }
    }
    h->n_rb_total = p.total;
    std::copy(p.start.begin(), p.start.end(), h->h_rb_start.begin());
    h->h_cap_rb = p.cap;
    return 0;
}

// 5 scatter: every new object after the last object of its bucket, in call order -- its id, then its row (add_rows_impl)
static int insert_scatter(lmi_index* h, const void* rows, int src16, const int64_t* labels, const uint32_t* ids, int64_t nrows, int on_device) {
    std::vector<int> pos((size_t)nrows);
    std::vector<int> fill(h->h_nb_rows);
    for (int64_t i = 0; i < nrows; ++i) {
        const int b = (int)labels[i];
        pos[i] = owns(h, b) ? h->h_rb_start[b] * 32 + fill[b]++ : -1;
    }
    HIPCHK(hipMemcpyAsync(h->mut_pos.p, pos.data(), (size_t)nrows * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->mut_ids.p, ids, (size_t)nrows * 4, hipMemcpyHostToDevice, h->stream));
    scatter_ids_kernel<<<cdiv(nrows, 256), 256, 0, h->stream>>>(h->mut_ids.as<uint32_t>(), h->mut_pos.as<int>(), nrows, h->ids_slab.as<uint32_t>());
    HIPCHK(hipGetLastError());
    return add_rows_impl(h, rows, src16, 0, nullptr, nrows, on_device, h->mut_pos.as<int>(), nrows);   // (synchronises after a host piece: pos may go)
}

// The row ranges a call touched, as the range lists of lmi_mutate.h: five lists of `stride` ints, [bucket | first row | rows | first
// row-block | row-blocks], n of them filled
struct RangeList {
    std::vector<int> v;
    int stride, n = 0, max_rows = 0, max_rb = 0;
    explicit RangeList(int stride_) : v((size_t)5 * stride_), stride(stride_) {}
    void add(int bucket, int row0, int nrows, int rb0, int nrb) {
        const int f[5] = {bucket, row0, nrows, rb0, nrb};
        for (int i = 0; i < 5; ++i) v[(size_t)i * stride + n] = f[i];
        max_rows = std::max(max_rows, nrows);
        max_rb = std::max(max_rb, nrb);
        ++n;
    }
    int conv_blocks(const lmi_index* h) const { return std::max(1, std::min(1024, cdiv((long long)max_rb * 32 * h->KG16 * 2, 256))); }
};

// 6 ranges: [n_old, n_new) of every bucket that received rows; the host tables take the rows in
static RangeList insert_ranges(lmi_index* h, const std::vector<int64_t>& add, const int64_t* labels, int64_t nrows) {
    const int L = h->L;
    RangeList r(L);
    for (int b = 0; b < L; ++b) {
        if (!add[b]) continue;
        const int r0 = h->h_rb_start[b] * 32 + h->h_nb_rows[b], r1 = r0 + (int)add[b];
        r.add(b, r0, r1 - r0, r0 / 32, cdiv(r1, 32) - r0 / 32);
        h->h_nb_rows[b] += (int)add[b];
        h->h_any[b] = 1;
    }
    for (int64_t i = 0; i < nrows; ++i) h->h_any[labels[i]] = 1;   // (buckets of other ranks too)
    h->N += nrows;
    return r;
}

// 7 images: what the prefilter derives from the rows, for the touched ranges -- or for the whole slab, when the new rows break
// max|x'| < 1 under the current scale (or no fp16 image exists yet)
static int insert_images(lmi_index* h, const RangeList& r) {
    HIPCHK(hipMemcpyAsync(h->mut_list.p, r.v.data(), r.v.size() * 4, hipMemcpyHostToDevice, h->stream));
    const int* d_list = h->mut_list.as<int>();
    bool rescale = !h->have16;
    if (!rescale) {   // the new rows' max |x| under the current scale
        HIPCHK(hipMemsetAsync(h->mut_word.p, 0, 4, h->stream));
        dim3 g(std::min(64, cdiv((long long)r.max_rows * h->d, 256)), r.n);
        absmax_ranges_kernel<<<g, 256, 0, h->stream>>>(h->rowmajor.as<float>(), h->d, h->dp, d_list + r.stride, d_list + 2 * r.stride, h->mut_word.as<unsigned>());
        HIPCHK(hipGetLastError());
        unsigned mbits = 0;
        float sc = 1.0f;
        HIPCHK(hipMemcpyAsync(&mbits, h->mut_word.p, 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipMemcpyAsync(&sc, h->xscale.p, 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        float m;
        memcpy(&m, &mbits, 4);
        rescale = !(m * sc < 1.0f);   // (exact: sc is a power of two)
    }
    if (rescale) return prefilter_images(h);   // a new scale: the whole fp16 slab and every bucket's maxima, as lmi_buckets_end
    return redo_ranges(h, d_list, r.stride, r.n, r.conv_blocks(h), r.max_rows);
}

// lmi_buckets_insert / lmi_buckets_insert_f16 (src16: the rows are halves; `who`: the entry point, for the refusals of mut_check)
static int insert_impl(lmi_index* h, const void* rows, int src16, const int64_t* labels, const uint32_t* ids, int64_t nrows,
                       int on_device, int64_t* n_stored, const char* who) {
    CHK(mut_check(h, who));
    if (nrows < 0 || (nrows > 0 && (!rows || !labels || !ids)))
        return fail("%s: bad arguments (rows, labels and ids are required; the ids are the caller's)", who);
    if (nrows >= (1ll << 31)) return fail("%s: %lld rows in one call (fewer than 2^31)", who, (long long)nrows);
    std::vector<int64_t> add;
    int64_t stored = 0;
    CHK(insert_count(h, labels, nrows, who, add, &stored));
    if (n_stored) *n_stored = 0;
    if (stored == 0) return 0;
    // 2 plan: the layout after the call (lmi_layout.h)
    const lmi_layout::InsertPlan plan = lmi_layout::plan_insert(h->h_nb_rows, h->h_rb_start, h->h_cap_rb, h->n_rb_total, add, h->chunk_rows / 32,
                                                                alloc_rb(h), lmi_layout::max_slab_rb(h->L));
    if (plan.refusal == lmi_layout::InsertPlan::BUCKET_PAST_LIMIT)
        return fail("%s: bucket %d would exceed the 32-bit positions of the slab", who, plan.bucket);
    if (plan.refusal == lmi_layout::InsertPlan::TOTAL_PAST_LIMIT)
        return fail("%s: %lld row-blocks of rows, spare row-blocks and holes exceed the 32-bit positions of the slab", who, (long long)plan.total);
    CHK(set_dev(h));
    CHK(insert_reserve(h, nrows, src16, on_device));
    HIPCHK(hipStreamSynchronize(h->stream));   // searches enqueued before the call read the index as it was
    h->layout_stamp = next_layout_stamp();     // from here on the slab changes: the filters made before the call are stale
    CHK(insert_relocate(h, plan));
    CHK(insert_scatter(h, rows, src16, labels, ids, nrows, on_device));
    const RangeList ranges = insert_ranges(h, add, labels, nrows);
    CHK(mut_derive(h));
    if (h->prefilter) CHK(insert_images(h, ranges));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int i = 0; i < 4; ++i) h->mut_paths[i] += plan.paths[i];
    if (n_stored) *n_stored = stored;
    return 0;
}

extern "C" LMI_API int lmi_buckets_insert(lmi_index* h, const float* rows, const int64_t* labels, const uint32_t* ids, int64_t nrows,
                                          int on_device, int64_t* n_stored) {
    return insert_impl(h, rows, 0, labels, ids, nrows, on_device, n_stored, "lmi_buckets_insert");
}
extern "C" LMI_API int lmi_buckets_insert_f16(lmi_index* h, const uint16_t* rows, const int64_t* labels, const uint32_t* ids, int64_t nrows,
                                              int on_device, int64_t* n_stored) {
    return insert_impl(h, rows, 1, labels, ids, nrows, on_device, n_stored, "lmi_buckets_insert_f16");
}

// ---- delete, step by step ----
// 4 compact: the hit buckets' kept rows, in order, into staging (groups of at most ~1 GiB, lmi_layout.h) and back in place, zeros to
// the end of the old row-blocks.  hit / span: the buckets that lose rows and the rows of their row-blocks; w->mut_keep: mark_rows' flags
static int delete_compact(lmi_index* h, const std::vector<int>& hit, const std::vector<int>& span) {
    const int nh = (int)hit.size();
    const bool frag = stored_form(h) == FORM_FRAG32;
    const int pitch = frag ? h->d : h->dp;
    const int64_t max_span = *std::max_element(span.begin(), span.end());
    const lmi_layout::DeleteGroups grp = lmi_layout::delete_groups(span, std::max<int64_t>(max_span, (1ll << 30) / ((int64_t)pitch * 4)));
    CHK(h->mut_stage.reserve((size_t)grp.stage_rows * pitch * 4 + (size_t)grp.stage_rows * 4));
    float* st_rows = h->mut_stage.as<float>();
    uint32_t* st_ids = reinterpret_cast<uint32_t*>(st_rows + (size_t)grp.stage_rows * pitch);
    // device lists: [hit | span] ints, then the buckets' staging offsets (8-byte aligned)
    std::vector<int> ilist(hit);
    ilist.insert(ilist.end(), span.begin(), span.end());
    const size_t off_bytes = rup((size_t)ilist.size() * 4, 8);
    HIPCHK(hipMemcpyAsync(h->mut_list.p, ilist.data(), ilist.size() * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->mut_list.as<char>() + off_bytes, grp.goff.data(), grp.goff.size() * 8, hipMemcpyHostToDevice, h->stream));
    const int *d_hit = h->mut_list.as<int>(), *d_span = d_hit + nh;
    const long long* d_goff = reinterpret_cast<const long long*>(h->mut_list.as<char>() + off_bytes);
    compact_map_kernel<<<nh, CM_THREADS, 0, h->stream>>>(d_hit, d_span, h->d_rb_start.as<int>(), h->d_nb_rows.as<int>(), h->mut_keep.as<int>(),
                                                        h->mut_src.as<int>());
    HIPCHK(hipGetLastError());
    const int per_row = frag ? cdiv(pitch, 8) : pitch / 4;
    for (int g = 0; g < grp.n(); ++g) {
        const int i0 = grp.gfirst[g], ng = grp.gfirst[g + 1] - i0;
        const int64_t gmax = *std::max_element(span.begin() + i0, span.begin() + i0 + ng);
        dim3 gg(std::max(1, std::min(1024, cdiv(gmax * per_row, 256))), ng);
        if (frag)
            gather_compact_kernel<true><<<gg, 256, 0, h->stream>>>(h->slab.as<float>(), pitch, h->KGs, h->ids_slab.as<uint32_t>(), d_hit + i0, d_goff + i0,
                                                                  d_span + i0, h->d_rb_start.as<int>(), h->mut_src.as<int>(), st_rows, st_ids);
        else
            gather_compact_kernel<false><<<gg, 256, 0, h->stream>>>(h->rowmajor.as<float>(), pitch, 0, h->ids_slab.as<uint32_t>(), d_hit + i0, d_goff + i0,
                                                                   d_span + i0, h->d_rb_start.as<int>(), h->mut_src.as<int>(), st_rows, st_ids);
        HIPCHK(hipGetLastError());
        for (int i = i0; i < i0 + ng; ++i) {   // back in place
            const size_t p0 = (size_t)h->h_rb_start[hit[i]] * 32;
            const long long sp = span[i], off = grp.goff[i];
            if (frag) {
                pack_gather_kernel<<<cdiv(sp * h->KGs, 256), 256, 0, h->stream>>>(st_rows + off * pitch, pitch, nullptr, (int)sp, sp, h->KGs,
                                                                                  h->slab.as<float4>() + (p0 >> 5) * h->KGs * 64);
                HIPCHK(hipGetLastError());
            } else {
                HIPCHK(hipMemcpyAsync(h->rowmajor.as<float>() + p0 * pitch, st_rows + off * pitch, (size_t)sp * pitch * 4, hipMemcpyDeviceToDevice, h->stream));
            }
            HIPCHK(hipMemcpyAsync(h->ids_slab.as<uint32_t>() + p0, st_ids + off, (size_t)sp * 4, hipMemcpyDeviceToDevice, h->stream));
        }
    }
    return 0;
}

extern "C" LMI_API int lmi_buckets_delete(lmi_index* h, const uint32_t* ids, int64_t n, int64_t* n_removed) {
    CHK(mut_check(h, "lmi_buckets_delete"));
    if (n < 0 || (n > 0 && !ids)) return fail("lmi_buckets_delete: bad arguments");
    if (n_removed) *n_removed = 0;
    if (n == 0 || h->owned_total == 0) return 0;
    const int L = h->L;
    CHK(set_dev(h));
    CHK(h->mut_list.reserve((size_t)L * 4 * 4 + (size_t)L * 8 + 16));
    CHK(h->mut_pos.reserve((size_t)L * 5 * 4));
    HIPCHK(hipStreamSynchronize(h->stream));   // searches enqueued before the call read the index as it was
    // 1-3: mark the rows whose id is not listed and count them per bucket; the buckets that lose rows
    std::vector<int> kept;
    CHK(mark_rows(h, h, ids, n, LMI_SUBSET_DROP, 0, kept));
    std::vector<int> hit, span;
    int64_t removed = 0;
    for (int b = 0; b < L; ++b)
        if (kept[b] < h->h_nb_rows[b]) {
            hit.push_back(b);
            span.push_back(cdiv(h->h_nb_rows[b], 32) * 32);
            removed += h->h_nb_rows[b] - kept[b];
        }
    if (removed == 0) return 0;
    h->layout_stamp = next_layout_stamp();   // from here on the slab changes: the filters made before the call are stale
    CHK(delete_compact(h, hit, span));
    // 5: the tables, then the hit buckets' fp16 row-blocks and maxima from their rows as they are now
    for (int b : hit) {
        h->h_nb_rows[b] = kept[b];
        if (kept[b] == 0) h->h_any[b] = 0;   // (the bucket is this handle's: no other rank holds rows of it)
    }
    h->N -= removed;
    CHK(mut_derive(h));
    const int nh = (int)hit.size();
    RangeList r(nh);   // (alive until the stream has taken it)
    if (stored_form(h) == FORM_ROWMAJOR && h->have16) {
        for (int i = 0; i < nh; ++i) r.add(hit[i], h->h_rb_start[hit[i]] * 32, kept[hit[i]], h->h_rb_start[hit[i]], span[i] / 32);
        HIPCHK(hipMemcpyAsync(h->mut_pos.p, r.v.data(), r.v.size() * 4, hipMemcpyHostToDevice, h->stream));
        const int* d_list = h->mut_pos.as<int>();
        reset_norms_kernel<<<cdiv(nh, 256), 256, 0, h->stream>>>(d_list, nh, h->bnorm.as<unsigned>(), h->bdelta.as<unsigned>());
        HIPCHK(hipGetLastError());
        CHK(redo_ranges(h, d_list, nh, nh, r.conv_blocks(h), std::max(1, r.max_rows)));
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    if (n_removed) *n_removed = removed;
    return 0;
}
