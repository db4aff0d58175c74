// lmi_host_mutate.h -- lmi_buckets_insert / lmi_buckets_delete on a built index (kernels: lmi_mutate.h).
#pragma once
#include "lmi_host_build.h"

// ------------------------------------------------------------------------------------------------
// Mutation of a built index (no reference counterpart: the reference rebuilds).  Bucket b holds h_nb_rows[b] rows from
// row-block h_rb_start[b] on and has h_cap_rb[b] row-blocks reserved there; the slab's first n_rb_total row-blocks are
// buckets, their spare row-blocks and holes (the old places of relocated buckets), all of them zero where no row lives.
// An insert that overflows a bucket's capacity moves the bucket behind the last row-block with slack; when that does not
// fit the allocations, or the holes would pass a quarter of the slab, every bucket is re-packed into new allocations.
// A handle that is never mutated keeps lmi_buckets_end's layout byte for byte.
namespace {
struct SlabImage { DevBuf* buf; size_t rb_bytes, extra; };
int slab_images(lmi_index* h, SlabImage* im) {   // every per-row image the mode keeps, row-block-major
    int n = 0;
    if (h->prefilter) {
        im[n++] = {&h->rowmajor, (size_t)32 * h->dp * 4, 0};
        if (h->have16) im[n++] = {&h->slab16, (size_t)h->KG16 * 1024, 8192};   // + pass 2's look-ahead (lmi_buckets_end)
    } else {
        im[n++] = {&h->slab, (size_t)h->KGs * 1024, 0};
    }
    im[n++] = {&h->ids_slab, 128, 0};
    return n;
}
int64_t alloc_rb(lmi_index* h) {   // row-blocks every image's allocation holds
    SlabImage im[3];
    const int n = slab_images(h, im);
    int64_t a = INT64_MAX;
    for (int i = 0; i < n; ++i) a = std::min<int64_t>(a, im[i].buf->cap < im[i].extra ? 0 : (int64_t)((im[i].buf->cap - im[i].extra) / im[i].rb_bytes));
    return a;
}
int64_t max_slab_rb(const lmi_index* h) { return ((1ll << 31) - 64ll * h->L) / 32 - 1; }   // lmi_buckets_begin's limit on positions
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
    int max_rows = 0, nonempty = 0;
    h->owned_total = 0;
    for (int b = 0; b < L; ++b) {
        max_rows = std::max(max_rows, h->h_nb_rows[b]);
        h->owned_total += h->h_nb_rows[b];
        nonempty += h->h_any[b] || h->h_nb_rows[b] > 0;
    }
    h->n_nonempty = std::max(1, nonempty);
    const int need = (int)rup(cdiv(max_rows, 1024), 256);   // a bucket is scanned in at most 1024 chunks (lmi_buckets_begin)
    if (need > h->chunk_rows) h->chunk_rows = need;
    const int chunk_rb = h->chunk_rows / 32;
    for (int b = 0; b < L; ++b) h->h_nch[b] = cdiv(cdiv(h->h_nb_rows[b], 32), chunk_rb);
    h->h_rb_start[L] = (int)h->n_rb_total;
    HIPCHK(hipMemcpyAsync(h->d_nb_rows.p, h->h_nb_rows.data(), L * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_rb_start.p, h->h_rb_start.data(), (L + 1) * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_nch.p, h->h_nch.data(), L * 4, hipMemcpyHostToDevice, h->stream));
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
    SlabImage im[3];
    const int n = slab_images(h, im);
    DevBuf fresh[3];   // (an early return frees them)
    size_t bytes[3] = {0, 0, 0};
    for (int i = 0; i < n; ++i) {
        bytes[i] = (size_t)std::max<int64_t>(alloc_new, 1) * im[i].rb_bytes + im[i].extra;
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

// lmi_buckets_insert / lmi_buckets_insert_f16 (src16: the rows are halves; `who`: the entry point, for the refusals of mut_check)
static int insert_impl(lmi_index* h, const void* rows, int src16, const int64_t* labels, const uint32_t* ids, int64_t nrows,
                       int on_device, int64_t* n_stored, const char* who) {
    CHK(mut_check(h, who));
    if (nrows < 0 || (nrows > 0 && (!rows || !labels || !ids)))
        return fail("%s: bad arguments (rows, labels and ids are required; the ids are the caller's)", who);
    if (nrows >= (1ll << 31)) return fail("%s: %lld rows in one call (fewer than 2^31)", who, (long long)nrows);
    const int L = h->L;
    std::vector<int64_t> add(L, 0);
    int64_t stored = 0;
    for (int64_t i = 0; i < nrows; ++i) {
        const int64_t b = labels[i];
        if (b < 0 || b >= L) return fail("%s: labels[%lld] = %lld outside [0,%d); nothing was inserted", who, (long long)i, (long long)b, L);
        if (owns(h, (int)b)) { add[b]++; stored++; }
    }
    if (n_stored) *n_stored = 0;
    if (stored == 0) return 0;
    // the layout after the call: buckets that outgrow their row-blocks move behind the last one with geometric slack
    const int chunk_rb = h->chunk_rows / 32;
    std::vector<int> start(h->h_rb_start.begin(), h->h_rb_start.begin() + L), cap = h->h_cap_rb;
    std::vector<unsigned char> moved(L, 0);
    int64_t tail = h->n_rb_total, used = 0;
    for (int b = 0; b < L; ++b) {
        const int64_t need = ((int64_t)h->h_nb_rows[b] + add[b] + 31) / 32;
        if (need > cap[b]) {
            // + a quarter (not x2: the images of a 10M x 768 index are 46 GB) and at least a chunk
            const int64_t c = need + std::max<int64_t>(need / 4, chunk_rb);
            if (c > max_slab_rb(h)) return fail("%s: bucket %d would exceed the 32-bit positions of the slab", who, b);
            cap[b] = (int)c;
            start[b] = (int)std::min<int64_t>(tail, INT32_MAX);
            moved[b] = 1;
            tail += c;
        }
        used += cap[b];
    }
    const int64_t have = alloc_rb(h);
    const bool pack = tail > have || (tail - used) * 4 > tail;   // grow, or reclaim holes past a quarter of the slab
    int64_t total = tail, alloc_new = have;
    if (pack) {
        total = 0;
        for (int b = 0; b < L; ++b) { start[b] = (int)std::min<int64_t>(total, INT32_MAX); total += cap[b]; }
        alloc_new = std::min(total + total / 8, max_slab_rb(h));
    }
    // which layout path ran (lmi_debug_layout).  A re-pack whose packed layout fits the allocations it replaces was forced by the
    // holes, not by the rows: with 1/8 headroom, holes never pass a quarter of the slab before the tail reaches the allocation's end
    int64_t paths[4] = {0, 0, 0, 0};
    if (pack) {
        paths[total > have ? 2 : 3] = 1;
    } else {
        for (int b = 0; b < L; ++b) paths[moved[b] ? 1 : 0] += add[b] > 0;
    }
    if (total > max_slab_rb(h))
        return fail("%s: %lld row-blocks of rows, spare row-blocks and holes exceed the 32-bit positions of the slab", who, (long long)total);
    CHK(set_dev(h));
    // every allocation the call needs before the first change (a failure leaves the index as it was)
    const int64_t piece = std::max<int64_t>(1, (256ll << 20) / ((int64_t)h->d * 4));   // add_rows_impl's pieces
    const int64_t np = std::min(piece, nrows);
    if (!on_device) CHK(h->stage.reserve((size_t)np * h->d_user * (src16 ? 2 : 4)));
    if (src16) CHK(h->wide.reserve((size_t)np * h->d_user * 4));
    if (h->metric == LMI_METRIC_L2) CHK(h->aug_rows.reserve((size_t)np * h->d * 4));
    CHK(h->mut_pos.reserve((size_t)nrows * 4));
    CHK(h->mut_ids.reserve((size_t)nrows * 4));
    CHK(h->mut_list.reserve((size_t)L * 5 * 4));
    CHK(h->mut_word.reserve(16));
    HIPCHK(hipStreamSynchronize(h->stream));   // searches enqueued before the call read the index as it was
    SlabImage im[3];
    const int nim = slab_images(h, im);
    if (pack) {
        std::vector<int> from(h->h_rb_start.begin(), h->h_rb_start.begin() + L);
        CHK(repack(h, from, start, h->h_cap_rb, alloc_new));
    } else {
        for (int b = 0; b < L; ++b) {
            if (!moved[b]) continue;
            const int from = h->h_rb_start[b], nrb = h->h_cap_rb[b];
            // old row-blocks to the new place, zeros after them (past n_rb_total an allocation holds whatever it held), and zeros
            // where they were (a hole: rescaling takes the absmax of every row-block of the layout)
            for (int i = 0; i < nim; ++i) {
                char* base = im[i].buf->as<char>();
                const size_t rb = im[i].rb_bytes;
                if (nrb > 0) {
                    HIPCHK(hipMemcpyAsync(base + (size_t)start[b] * rb, base + (size_t)from * rb, (size_t)nrb * rb, hipMemcpyDeviceToDevice, h->stream));
                    HIPCHK(hipMemsetAsync(base + (size_t)from * rb, 0, (size_t)nrb * rb, h->stream));
                }
                HIPCHK(hipMemsetAsync(base + (size_t)(start[b] + nrb) * rb, 0, (size_t)(cap[b] - nrb) * rb, h->stream));
            }
        }
    }
    h->n_rb_total = total;
    for (int b = 0; b < L; ++b) h->h_rb_start[b] = start[b];
    h->h_cap_rb = cap;
    // every new object after the last object of its bucket, in call order
    std::vector<int> pos((size_t)nrows);
    std::vector<int> fill(h->h_nb_rows);
    for (int64_t i = 0; i < nrows; ++i) {
        const int b = (int)labels[i];
        pos[i] = owns(h, b) ? start[b] * 32 + fill[b]++ : -1;
    }
    HIPCHK(hipMemcpyAsync(h->mut_pos.p, pos.data(), (size_t)nrows * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->mut_ids.p, ids, (size_t)nrows * 4, hipMemcpyHostToDevice, h->stream));
    scatter_ids_kernel<<<cdiv(nrows, 256), 256, 0, h->stream>>>(h->mut_ids.as<uint32_t>(), h->mut_pos.as<int>(), nrows, h->ids_slab.as<uint32_t>());
    HIPCHK(hipGetLastError());
    CHK(add_rows_impl(h, rows, src16, 0, nullptr, nrows, on_device, h->mut_pos.as<int>(), nrows));
    // the touched rows: [n_old, n_new) of every bucket that received some (range lists of lmi_mutate.h)
    std::vector<int> list((size_t)L * 5);
    int* l_b = list.data();
    int* l_row0 = l_b + L;
    int* l_nrows = l_row0 + L;
    int* l_rb0 = l_nrows + L;
    int* l_nrb = l_rb0 + L;
    int nr = 0, max_rows = 0, max_rb = 0;
    for (int b = 0; b < L; ++b) {
        if (!add[b]) continue;
        const int r0 = start[b] * 32 + h->h_nb_rows[b], r1 = r0 + (int)add[b];
        l_b[nr] = b;
        l_row0[nr] = r0;
        l_nrows[nr] = r1 - r0;
        l_rb0[nr] = r0 / 32;
        l_nrb[nr] = cdiv(r1, 32) - r0 / 32;
        max_rows = std::max(max_rows, l_nrows[nr]);
        max_rb = std::max(max_rb, l_nrb[nr]);
        ++nr;
        h->h_nb_rows[b] += (int)add[b];
        h->h_any[b] = 1;
    }
    for (int64_t i = 0; i < nrows; ++i) h->h_any[labels[i]] = 1;   // (buckets of other ranks too)
    h->N += nrows;
    CHK(mut_derive(h));
    if (h->prefilter) {
        HIPCHK(hipMemcpyAsync(h->mut_list.p, list.data(), list.size() * 4, hipMemcpyHostToDevice, h->stream));
        const int* d_list = h->mut_list.as<int>();
        bool rescale = !h->have16;
        if (!rescale) {   // the new rows' max |x| under the current scale: max|x'| < 1 must survive
            HIPCHK(hipMemsetAsync(h->mut_word.p, 0, 4, h->stream));
            dim3 g(std::min(64, cdiv((long long)max_rows * h->d, 256)), nr);
            absmax_ranges_kernel<<<g, 256, 0, h->stream>>>(h->rowmajor.as<float>(), h->d, h->dp, d_list + L, d_list + 2 * L, h->mut_word.as<unsigned>());
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
        if (rescale) {
            CHK(prefilter_images(h));   // a new scale: the whole fp16 slab and every bucket's maxima, as lmi_buckets_end
        } else {
            CHK(redo_ranges(h, d_list, L, nr, std::min(1024, cdiv((long long)max_rb * 32 * h->KG16 * 2, 256)), max_rows));
        }
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int i = 0; i < 4; ++i) h->mut_paths[i] += paths[i];
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

extern "C" LMI_API int lmi_buckets_delete(lmi_index* h, const uint32_t* ids, int64_t n, int64_t* n_removed) {
    CHK(mut_check(h, "lmi_buckets_delete"));
    if (n < 0 || (n > 0 && !ids)) return fail("lmi_buckets_delete: bad arguments");
    if (n_removed) *n_removed = 0;
    if (n == 0 || h->owned_total == 0) return 0;
    std::vector<uint32_t> del(ids, ids + n);
    std::sort(del.begin(), del.end());
    del.erase(std::unique(del.begin(), del.end()), del.end());
    const int L = h->L;
    const int64_t slab_rows = h->n_rb_total * 32;
    CHK(set_dev(h));
    CHK(h->mut_ids.reserve(del.size() * 4));
    CHK(h->mut_keep.reserve((size_t)slab_rows * 4));
    CHK(h->mut_src.reserve((size_t)slab_rows * 4));
    CHK(h->mut_word.reserve((size_t)L * 4));
    CHK(h->mut_list.reserve((size_t)L * 4 * 4 + (size_t)L * 8 + 16));
    CHK(h->mut_pos.reserve((size_t)L * 5 * 4));
    HIPCHK(hipStreamSynchronize(h->stream));   // searches enqueued before the call read the index as it was
    // 1-3: mark the rows whose id is listed and count them per bucket; the counts come back to the host
    HIPCHK(hipMemcpyAsync(h->mut_ids.p, del.data(), del.size() * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemsetAsync(h->mut_word.p, 0, (size_t)L * 4, h->stream));
    int max_n = 0;
    for (int b = 0; b < L; ++b) max_n = std::max(max_n, h->h_nb_rows[b]);
    mark_deleted_kernel<<<dim3(std::max(1, std::min(64, cdiv(max_n, 256))), L), 256, 0, h->stream>>>(
        h->ids_slab.as<uint32_t>(), h->d_rb_start.as<int>(), h->d_nb_rows.as<int>(), h->mut_ids.as<uint32_t>(), (int)del.size(),
        h->mut_keep.as<int>(), h->mut_word.as<int>());
    HIPCHK(hipGetLastError());
    std::vector<int> cnt(L);
    HIPCHK(hipMemcpyAsync(cnt.data(), h->mut_word.p, (size_t)L * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    std::vector<int> hit, span;
    int64_t removed = 0, max_span = 0;
    for (int b = 0; b < L; ++b)
        if (cnt[b] > 0) {
            hit.push_back(b);
            span.push_back(cdiv(h->h_nb_rows[b], 32) * 32);
            max_span = std::max<int64_t>(max_span, span.back());
            removed += cnt[b];
        }
    if (removed == 0) return 0;
    const int nh = (int)hit.size();
    // 4: stable compaction of the hit buckets -- their rows in order into staging (groups of at most ~1 GiB), then back
    const bool frag = !h->prefilter;
    const int pitch = frag ? h->d : h->dp;
    const int64_t budget = std::max<int64_t>(max_span, (1ll << 30) / ((int64_t)pitch * 4));
    std::vector<int> gb, gspan, gfirst;
    std::vector<long long> goff;
    int64_t acc = 0;
    for (int i = 0; i < nh; ++i) {
        if (i == 0 || acc + span[i] > budget) { gfirst.push_back(i); acc = 0; }
        gb.push_back(hit[i]);
        gspan.push_back(span[i]);
        goff.push_back(acc);
        acc += span[i];
    }
    gfirst.push_back(nh);
    int64_t stage_rows = 0;
    for (size_t g = 0; g + 1 < gfirst.size(); ++g) {
        int64_t s = 0;
        for (int i = gfirst[g]; i < gfirst[g + 1]; ++i) s += gspan[i];
        stage_rows = std::max(stage_rows, s);
    }
    CHK(h->mut_stage.reserve((size_t)stage_rows * pitch * 4 + (size_t)stage_rows * 4));
    float* st_rows = h->mut_stage.as<float>();
    uint32_t* st_ids = reinterpret_cast<uint32_t*>(st_rows + (size_t)stage_rows * pitch);
    // device lists: [hit | span | group buckets | group spans] ints, then the group offsets (8-byte aligned)
    std::vector<int> ilist((size_t)4 * nh + 2);
    std::copy(hit.begin(), hit.end(), ilist.begin());
    std::copy(span.begin(), span.end(), ilist.begin() + nh);
    std::copy(gb.begin(), gb.end(), ilist.begin() + 2 * nh);
    std::copy(gspan.begin(), gspan.end(), ilist.begin() + 3 * nh);
    const size_t off_bytes = rup((size_t)ilist.size() * 4, 8);
    HIPCHK(hipMemcpyAsync(h->mut_list.p, ilist.data(), ilist.size() * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->mut_list.as<char>() + off_bytes, goff.data(), goff.size() * 8, hipMemcpyHostToDevice, h->stream));
    const int* d_hit = h->mut_list.as<int>();
    const long long* d_goff = reinterpret_cast<const long long*>(h->mut_list.as<char>() + off_bytes);
    compact_map_kernel<<<nh, CM_THREADS, 0, h->stream>>>(d_hit, d_hit + nh, h->d_rb_start.as<int>(), h->d_nb_rows.as<int>(), h->mut_keep.as<int>(),
                                                        h->mut_src.as<int>());
    HIPCHK(hipGetLastError());
    const int per_row = frag ? cdiv(pitch, 8) : pitch / 4;
    for (size_t g = 0; g + 1 < gfirst.size(); ++g) {
        const int i0 = gfirst[g], ng = gfirst[g + 1] - i0;
        int64_t gmax = 0;
        for (int i = i0; i < i0 + ng; ++i) gmax = std::max<int64_t>(gmax, gspan[i]);
        dim3 gg(std::max(1, std::min(1024, cdiv(gmax * per_row, 256))), ng);
        if (frag)
            gather_compact_kernel<true><<<gg, 256, 0, h->stream>>>(h->slab.as<float>(), pitch, h->KGs, h->ids_slab.as<uint32_t>(), d_hit + 2 * nh + i0,
                                                                  d_goff + i0, d_hit + 3 * nh + i0, h->d_rb_start.as<int>(), h->mut_src.as<int>(), st_rows, st_ids);
        else
            gather_compact_kernel<false><<<gg, 256, 0, h->stream>>>(h->rowmajor.as<float>(), pitch, 0, h->ids_slab.as<uint32_t>(), d_hit + 2 * nh + i0,
                                                                   d_goff + i0, d_hit + 3 * nh + i0, h->d_rb_start.as<int>(), h->mut_src.as<int>(), st_rows, st_ids);
        HIPCHK(hipGetLastError());
        for (int i = i0; i < i0 + ng; ++i) {   // back in place: the kept rows first, zeros to the end of the old row-blocks
            const int b = gb[i];
            const size_t p0 = (size_t)h->h_rb_start[b] * 32;
            const long long sp = gspan[i], off = goff[i];
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
    std::vector<int> old_nrb(nh);
    for (int i = 0; i < nh; ++i) {
        const int b = hit[i];
        old_nrb[i] = span[i] / 32;
        h->h_nb_rows[b] -= cnt[b];
        if (h->h_nb_rows[b] == 0) h->h_any[b] = 0;   // (the bucket is this handle's: no other rank holds rows of it)
    }
    h->N -= removed;
    CHK(mut_derive(h));
    std::vector<int> list((size_t)5 * nh);   // (alive until the stream has taken it)
    if (h->prefilter && h->have16) {   // the hit buckets' fp16 row-blocks and maxima from their rows as they are now
        for (int i = 0; i < nh; ++i) {
            const int b = hit[i];
            list[i] = b;
            list[nh + i] = h->h_rb_start[b] * 32;
            list[2 * nh + i] = h->h_nb_rows[b];
            list[3 * nh + i] = h->h_rb_start[b];
            list[4 * nh + i] = old_nrb[i];
        }
        HIPCHK(hipMemcpyAsync(h->mut_pos.p, list.data(), list.size() * 4, hipMemcpyHostToDevice, h->stream));
        const int* d_list = h->mut_pos.as<int>();
        reset_norms_kernel<<<cdiv(nh, 256), 256, 0, h->stream>>>(d_list, nh, h->bnorm.as<unsigned>(), h->bdelta.as<unsigned>());
        HIPCHK(hipGetLastError());
        int max_rb = 0, max_rows = 1;
        for (int i = 0; i < nh; ++i) { max_rb = std::max(max_rb, old_nrb[i]); max_rows = std::max(max_rows, list[2 * nh + i]); }
        CHK(redo_ranges(h, d_list, nh, nh, std::max(1, std::min(1024, cdiv((long long)max_rb * 32 * h->KG16 * 2, 256))), max_rows));
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    if (n_removed) *n_removed = removed;
    return 0;
}
