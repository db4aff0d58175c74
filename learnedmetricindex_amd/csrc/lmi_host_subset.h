// lmi_host_subset.h -- lmi_subset: a second, independent index that holds some of a built index's objects (kernels: lmi_subset.h).
#pragma once
#include "lmi_host_mutate.h"
#include "lmi_subset.h"

// ------------------------------------------------------------------------------------------------
// No reference counterpart (the reference filters its DataFrames and rebuilds).  The new handle is what lmi_create + the source's
// settings + lmi_buckets_begin / add_rows / end over "every bucket's kept objects, in the order the source holds them" would be, made on
// the device: the rows are marked against the id list and counted per bucket, the host lays the new index out from the counts
// (begin_layout, lmi_host_build.h), the kept rows are gathered from the source's slabs straight into the new ones, and what a build
// derives from the rows is derived from the new handle's own rows.  The source is only read.
namespace {
// a copy of one packed Linear stack: allocations of pack_model's sizes, the weights device to device
int copy_model(hipStream_t st, const Model& s, Model& t) {
    t.dims = s.dims; t.n_rb = s.n_rb; t.KG = s.KG;
    t.Wf.assign(s.n_layers, DevBuf());
    t.bias.assign(s.n_layers, DevBuf());
    for (int i = 0; i < s.n_layers; ++i) {
        const size_t wb = (size_t)s.n_rb[i] * s.KG[i] * 1024, bb = (size_t)s.n_rb[i] * 32 * sizeof(float);
        CHK(t.Wf[i].reserve(wb));
        CHK(t.bias[i].reserve(bb));
        HIPCHK(hipMemcpyAsync(t.Wf[i].p, s.Wf[i].p, wb, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipMemcpyAsync(t.bias[i].p, s.bias[i].p, bb, hipMemcpyDeviceToDevice, st));
    }
    t.n_layers = s.n_layers;
    return 0;
}
int copy_table(hipStream_t st, const DevBuf& src, size_t bytes, DevBuf& dst) {
    CHK(dst.reserve(bytes));
    HIPCHK(hipMemcpyAsync(dst.p, src.p, bytes, hipMemcpyDeviceToDevice, st));
    return 0;
}
// What a derived index (lmi_subset, lmi_regroup, lmi_concat) takes over from the built index h it is derived from, on c's stream: h's
// settings (lmi_create read the environment's again) and chunk rule, copies of all its models and -- with_tree -- of the tree tables
// (the device descriptors point at the weights: rebuilt at the first use).
int inherit_handle(const lmi_index* h, lmi_index* c, bool with_tree) {
    hipStream_t st = c->stream;
    static_cast<Settings&>(*c) = *h;
    c->storage_req = h->storage;
    if (!h->chunk_rows_auto) c->chunk_rows = h->chunk_rows_set;
    c->models.resize(h->models.size());
    for (size_t m = 0; m < h->models.size(); ++m) CHK(copy_model(st, h->models[m], c->models[m]));
    c->tree_set = false;
    if (with_tree && h->tree_set) {
        c->h_child_offset = h->h_child_offset; c->h_child_model = h->h_child_model; c->h_child_bucket = h->h_child_bucket;
        const size_t total = h->h_child_model.size();
        CHK(copy_table(st, h->d_child_offset, h->h_child_offset.size() * 4, c->d_child_offset));
        CHK(copy_table(st, h->d_child_model, std::max<size_t>(total, 1) * 4, c->d_child_model));
        CHK(copy_table(st, h->d_child_bucket, std::max<size_t>(total, 1) * 4, c->d_child_bucket));
        c->tree_set = true;
    }
    c->desc_dirty = true;
    return 0;
}
// blocks of a grid-stride gather over `pieces` 16-byte pieces: enough waves to keep every CU's memory pipe busy, no more than the work
int gather_blocks(const lmi_index* h, long long pieces) { return (int)std::max<long long>(1, std::min<long long>((pieces + 255) / 256, (long long)h->num_cus * 32)); }
}  // namespace

// everything of lmi_subset behind the argument checks: fills the fresh handle c from h (h->stream is idle; c runs on the NULL stream)
static int subset_fill(lmi_index* h, lmi_index* c, const uint32_t* ids, int64_t n, int mode, int64_t* n_kept) {
    const int L = h->L;
    hipStream_t st = c->stream;
    // ---- h's settings, the models and the tree: copies of its own ----
    CHK(inherit_handle(h, c, true));
    // ---- 1: mark the rows that stay and count them per bucket; the counts come back to the host (16 zeroed bytes behind them: the
    //         fp16 gather's maximum) ----
    std::vector<int> cnt, iota(L);   // (iota: compact_map_kernel's bucket list; alive until the stream has taken it)
    CHK(mark_rows(h, c, ids, n, mode, 16, cnt));
    int64_t kept = 0;
    for (int b = 0; b < L; ++b) kept += cnt[b];
    // ---- 2: the layout of a fresh build of the kept objects.  An owned bucket that is left empty holds rows on no rank any more
    //         (lmi_buckets_delete's rule); the buckets of other ranks keep h's word ----
    std::vector<unsigned char> any(L, 0);
    for (int b = 0; b < L; ++b) any[b] = owns(h, b) ? cnt[b] > 0 : h->h_any[b];
    CHK(begin_layout(c, h->N - (h->owned_total - kept), h->d_user, L, cnt.data(), any.data(), h->h_owned.empty() ? nullptr : h->h_owned.data(),
                     "lmi_subset"));
    if (c->d != h->d || c->dp != h->dp || c->KGs != h->KGs || (c->prefilter && c->storage == LMI_STORAGE_F16 && (c->KG16 != h->KG16 || frag16x16(c) != frag16x16(h))))
        return fail("internal: the new handle's images are shaped differently from the source's (%s:%d)", __FILE__, __LINE__);
    const int64_t new_rows = c->n_rb_total * 32;
    HIPCHK(hipMemsetAsync(c->ids_slab.p, 0, (size_t)std::max<int64_t>(c->n_rb_total, 1) * 32 * 4, st));
    if (kept > 0) {
        // ---- 3: the stable source map: every bucket's kept rows in order (compact_map_kernel over all buckets, in h's layout), then
        //         per row of the NEW slab the slab row of h it comes from (-1 behind a bucket's last row) ----
        for (int b = 0; b < L; ++b) iota[b] = b;
        HIPCHK(hipMemcpyAsync(c->mut_list.p, iota.data(), (size_t)L * 4, hipMemcpyHostToDevice, st));
        compact_map_kernel<<<L, CM_THREADS, 0, st>>>(c->mut_list.as<int>(), h->d_nb_rows.as<int>(), h->d_rb_start.as<int>(), h->d_nb_rows.as<int>(),
                                                    c->mut_keep.as<int>(), c->mut_src.as<int>());
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemsetAsync(c->mut_keep.p, 0xFF, (size_t)new_rows * 4, st));   // (no more rows than h's slab, which mut_keep was sized for: no bucket grows)
        int max_n = 0;
        for (int b = 0; b < L; ++b) max_n = std::max(max_n, cnt[b]);
        subset_srcpos_kernel<<<dim3(std::max(1, std::min(64, cdiv(max_n, 256))), L), 256, 0, st>>>(
            h->d_rb_start.as<int>(), c->mut_src.as<int>(), c->d_rb_start.as<int>(), c->d_nb_rows.as<int>(), c->mut_keep.as<int>());
        HIPCHK(hipGetLastError());
        const int* srcpos = c->mut_keep.as<int>();
        // ---- 4: the gather of the stored image, the ids alongside ----
        switch (stored_form(c)) {
        case FORM_FRAG16: {
            const long long pieces = c->n_rb_total * c->KG16 * 64;
            unsigned* maxbits = c->mut_word.as<unsigned>() + L;   // (zeroed by mark_rows)
            subset_gather_frag16_kernel<<<gather_blocks(c, pieces), 256, 0, st>>>(h->slab16.as<uint4>(), h->ids_slab.as<uint32_t>(), srcpos, c->n_rb_total,
                                                                                   c->KG16, frag16x16(c), c->slab16.as<uint4>(), c->ids_slab.as<uint32_t>(),
                                                                                   maxbits);
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
        // the stored halves are x * s_old; the kept rows' own scale s_new >= s_old, and the pieces times the power of two s_new / s_old
        // are the halves x * s_new a fresh build stores (exact: the product is below 1 and only moves the exponent up)
        CHK(c->mut_stage.reserve(16));
        CHK(storage16_images(c, c->mut_stage, [&]() -> int {
            subset_scale16_kernel<<<1, 1, 0, st>>>(c->mut_word.as<unsigned>() + L, h->xscale.as<float>(), c->xmaxbits.as<unsigned>(), c->xscale.as<float>(),
                                                  c->mut_stage.as<float>());
            HIPCHK(hipGetLastError());
            return 0;
        }));
        c->have16 = true;
    } else if (c->prefilter && c->n_rb_total > 0) {
        CHK(prefilter_images(c));   // its own absmax, scale, fp16 fragments and norms
    }
    unsigned st16[2] = {0u, 0u};   // LMI_STORAGE_F16: [1] = the S16_* flags the rescale raised (none, by the argument above)
    if (c->have16 && c->storage == LMI_STORAGE_F16) HIPCHK(hipMemcpyAsync(st16, c->xmaxbits.p, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (st16[1]) return fail("internal: bringing the kept halves to the subset's scale was not exact (flags %u)", st16[1]);
    for (DevBuf* b : {&c->mut_ids, &c->mut_keep, &c->mut_src, &c->mut_word, &c->mut_list, &c->mut_stage}) b->release();   // the call's maps
    c->building = false;
    c->built = true;
    c->layout_stamp = next_layout_stamp();   // its own layout: no filter of the source fits it
    if (n_kept) *n_kept = kept;
    return 0;
}

extern "C" LMI_API int lmi_subset(lmi_index* h, const uint32_t* ids, int64_t n, int mode, lmi_index** out, int64_t* n_kept) {
    if (!out) return fail("lmi_subset: out is NULL");
    *out = nullptr;
    if (n_kept) *n_kept = 0;
    if (!h) return fail("lmi_subset: NULL handle");
    if (h->building) return fail("lmi_subset: the index is being built (lmi_buckets_end has not run)");
    if (!h->built) return fail("lmi_subset: the bucket index is not built (lmi_buckets_end has not run)");
    if (mode != LMI_SUBSET_KEEP && mode != LMI_SUBSET_DROP)
        return fail("lmi_subset: unknown mode %d (LMI_SUBSET_KEEP = 0, LMI_SUBSET_DROP = 1)", mode);
    if (n < 0 || (n > 0 && !ids)) return fail("lmi_subset: bad arguments (n >= 0; ids is required when n > 0)");
    CHK(set_dev(h));
    HIPCHK(hipStreamSynchronize(h->stream));   // what was enqueued on h before the call (a build's tail, a mutation) is in the slabs
    lmi_index* c = nullptr;
    if (lmi_create(h->device, &c) != 0) return fail("lmi_subset: %s", std::string(g_err).c_str());
    if (subset_fill(h, c, ids, n, mode, n_kept) != 0) {   // the new handle and everything the call allocated go; h was only read
        const std::string why = g_err;
        (void)hipStreamSynchronize(c->stream);
        (void)lmi_destroy(c);
        if (n_kept) *n_kept = 0;
        return fail("lmi_subset: %s; no index was made and the source is unchanged", why.c_str());
    }
    *out = c;
    return 0;
}
