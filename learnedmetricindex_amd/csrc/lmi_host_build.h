// lmi_host_build.h -- building the bucket index (lmi_buckets_begin / add_rows / end), the prefilter's images of the slab, and reading
// a bucket back.
#pragma once
#include "lmi_host.h"

// k16-groups of the fp16 fragments of d-column vectors (pass2_kernel's stages hold two k16-groups; the low-dimensional form has no
// stages: d = 45 is 48 wide, not 64)
static int kg16_for(const lmi_index* h, int d) {
    return low_d_form(h, cdiv(d, 16)) ? (int)cdiv(d, 16) : (int)rup(cdiv(d, 16), PF_STAGE_G);
}
// bytes of the fp16 fragments (with pass 2's look-ahead behind them, lmi_host.h)
static size_t slab16_bytes(const lmi_index* h) { return (size_t)std::max<int64_t>(h->n_rb_total, 1) * h->KG16 * 1024 + P2_LOOKAHEAD_BYTES; }

// owned_total / n_nonempty / chunk_rows / h_nch from h_nb_rows and h_any (lmi_layout.h); pick: a build's automatic chunk length
static void derive_tables(lmi_index* h, const lmi_layout::AutoChunk* pick) {
    const lmi_layout::Tables t = lmi_layout::derive_tables(h->h_nb_rows, h->h_any, h->chunk_rows, pick, h->h_nch);
    h->owned_total = t.owned_total;
    h->n_nonempty = t.n_nonempty;
    h->chunk_rows = t.chunk_rows;
}

// The part of lmi_buckets_begin that follows from the per-bucket counts alone (lmi_subset starts here: it knows how many objects every
// bucket keeps, not a label array): the handle's shape, the chunk length, the layout, the zero-filled images and the device copies of the
// bucket tables.  counts[L]: the rows this handle stores per bucket (0 for a bucket it does not own); any[L]: the bucket holds rows on some
// rank; owned: lmi_buckets_begin's (nullable).  The ids' image is reserved, not filled; the caller marks the handle `building`.
static int begin_checks(lmi_index* h, int64_t N, int L, const char* who) {
    if (h->storage_req == LMI_STORAGE_F16)
        if (const char* why = storage16_conflict(h)) return fail("%s: LMI_STORAGE_F16: %s", who, why);
    if (N >= (1ll << 31) - 64ll * L) return fail("%s: N too large for 32-bit positions", who);
    if (L >= (1 << ROUTE_ID_BITS)) return fail("%s: %d buckets, the routing kernels take fewer than %d", who, L, 1 << ROUTE_ID_BITS);
    return 0;
}
static int begin_layout(lmi_index* h, int64_t N, int d, int L, const int* counts, const unsigned char* any, const uint8_t* owned,
                        const char* who) {
    CHK(begin_checks(h, N, L, who));
    CHK(set_dev(h));
    if (h->storage_req == LMI_STORAGE_F16) CHK(storage16_kernel_attrs(h));
    h->N = N;
    h->d_user = d;
    h->d = h->metric == LMI_METRIC_L2 ? (int)rup(d + 1, 4) : d;  // L2: + the -|x|^2/2 column (sim_to_dist, lmi_kernels.h)
    d = h->d;
    h->dp = (int)rup(d, 4);   // floats per row of the row-major f32 copy: 16-byte rows for the streamed re-rank (d = 45: 48, zero-filled)
    h->storage = h->storage_req;
    if (h->storage == LMI_STORAGE_F16) h->dp = (int)rup(d, 8);   // no such copy: the floats of a query the re-rank stages (whole 8-k pieces)
    h->have16 = false;
    h->L = L;
    h->KGs = (int)rup(cdiv(d, 8), STAGE_G);
    h->built = false;
    h->h_nb_rows.assign(counts, counts + L);
    h->h_any.assign(any, any + L);
    if (owned) h->h_owned.assign(owned, owned + L);
    else h->h_owned.clear();
    // chunk rows not set by the caller: picked by the index size (lmi_layout.h); the layout of a build has no slack
    const lmi_layout::AutoChunk pick = {d, low_d_form(h, cdiv(d, 16)), h->prefilter};
    derive_tables(h, h->chunk_rows_auto ? &pick : nullptr);
    h->n_rb_total = lmi_layout::fresh_layout(h->h_nb_rows, h->h_rb_start, h->h_cap_rb);
    // the form's images, the others released.  Zero-filled where the rows arrive piece by piece (LMI_STORAGE_F16: unscaled until
    // lmi_buckets_end).  The fp16 fragments of the row-major form are reserved with the build's other images, so that a build that cannot
    // fit fails before the rows are uploaded and lmi_index_bytes reports the index's size from here on; lmi_buckets_end fills them.
    if (h->prefilter) h->KG16 = kg16_for(h, d);
    SlabImage im[MAX_SLAB_IMAGES];
    const int nim = slab_images(h, im, true);
    for (DevBuf* unused : {&h->slab, &h->rowmajor, &h->slab16})
        if (std::none_of(im, im + nim, [&](const SlabImage& i) { return i.buf == unused; })) unused->release();
    for (int i = 0; i < nim; ++i) {
        CHK(im[i].buf->reserve(im[i].bytes(h->n_rb_total)));
        if (im[i].zeroed) HIPCHK(hipMemsetAsync(im[i].buf->p, 0, im[i].bytes(h->n_rb_total), h->stream));
    }
    if (h->storage == LMI_STORAGE_F16) {
        CHK(h->xmaxbits.reserve(16));   // [0] max |x| (bits), [1] S16_* flags
        HIPCHK(hipMemsetAsync(h->xmaxbits.p, 0, 16, h->stream));
    }
    CHK(h->d_nb_rows.reserve(L * 4));
    CHK(h->d_rb_start.reserve((L + 1) * 4));
    CHK(h->d_nch.reserve(L * 4));
    HIPCHK(hipMemcpy(h->d_nb_rows.p, h->h_nb_rows.data(), L * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->d_rb_start.p, h->h_rb_start.data(), (L + 1) * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->d_nch.p, h->h_nch.data(), L * 4, hipMemcpyHostToDevice));
    h->rows_added = 0;
    h->indexed_ingest = false;
    return 0;
}

extern "C" LMI_API int lmi_buckets_begin(lmi_index* h, int64_t N, int d, int L, const int64_t* labels,
                                 const uint32_t* ids, const uint8_t* owned) {
    if (!h) return fail("lmi_buckets_begin: NULL handle");
    if (N < 0 || d < 1 || L < 1 || (N > 0 && !labels)) return fail("lmi_buckets_begin: bad arguments");
    CHK(begin_checks(h, N, L, "lmi_buckets_begin"));   // (first, as ever: a build that cannot be is refused before its labels are read)
    h->built = false;                                   // (from here on the handle holds no index, also when a label is refused below)
    std::vector<int> counts(L, 0);
    std::vector<unsigned char> any(L, 0);   // (a sharded rank: which buckets hold rows on ANY rank)
    for (int64_t i = 0; i < N; ++i) {
        int64_t b = labels[i];
        if (b < 0 || b >= L) return fail("lmi_buckets_begin: labels[%lld] = %lld outside [0,%d)", (long long)i, (long long)b, L);
        if (!owned || owned[b]) counts[b]++;
        any[b] = 1;
    }
    CHK(begin_layout(h, N, d, L, counts.data(), any.data(), owned, "lmi_buckets_begin"));
    // bucket-contiguous position of every object (stable: ascending original row inside a bucket,
    // the order pandas groupby yields) and the id of every slab row
    std::vector<int> pos((size_t)N);
    std::vector<uint32_t> ids_slab((size_t)std::max<int64_t>(h->n_rb_total, 1) * 32, 0u);
    std::vector<int> fill(L, 0);
    for (int64_t i = 0; i < N; ++i) {
        int b = (int)labels[i];
        if (owned && !owned[b]) { pos[i] = -1; continue; }
        int p = h->h_rb_start[b] * 32 + fill[b]++;
        pos[i] = p;
        ids_slab[p] = ids ? ids[i] : (uint32_t)(i + 1);  // search.py:190-191: 1-based labels
    }
    HIPCHK(hipMemcpy(h->ids_slab.p, ids_slab.data(), ids_slab.size() * 4, hipMemcpyHostToDevice));
    CHK(h->pos.reserve(std::max<size_t>(pos.size(), 1) * 4));
    if (N) HIPCHK(hipMemcpy(h->pos.p, pos.data(), pos.size() * 4, hipMemcpyHostToDevice));
    h->building = true;
    return 0;
}

// rows [nrows][d] are objects row0.. (index == NULL) or objects index[0..nrows) (host or device like `rows`)
// pos: slab row of every object (-1: not stored), n_total: its length (lmi_buckets_insert passes the batch's)
// src16: the rows are halves (uint16 bit patterns; the *_f16 entry points).  The piece size in ROWS is the same for both types, so a
// half piece stages half the bytes.  LMI_STORAGE_F16 takes the staged halves as they are (ingest16_half_kernel: no binary32 copy of
// the piece exists); LMI_STORAGE_F32 widens the piece once (widen16_kernel -> h->wide) and goes on as if it had arrived as floats.
// An ingest piece: 256 MiB of stored rows.  What a piece of n rows needs reserved: the staging of a host piece (its rows, then its
// index entries 8-byte aligned), the binary32 form of a half piece for an LMI_STORAGE_F32 index, the piece with its norm column (L2).
static int64_t ingest_piece_rows(const lmi_index* h) { return std::max<int64_t>(1, (256ll << 20) / ((int64_t)h->d * 4)); }
static size_t piece_index_offset(const lmi_index* h, int64_t n, int src16) {
    const size_t row_bytes = (size_t)n * h->d_user * (src16 ? 2 : 4);
    return src16 ? (size_t)rup((long long)row_bytes, 8) : row_bytes;
}
static int ingest_piece_reserve(lmi_index* h, int64_t n, int src16, bool indexed, int on_device) {
    if (!on_device) CHK(h->stage.reserve(piece_index_offset(h, n, src16) + (indexed ? (size_t)n * 8 : 0)));
    if (src16 && h->storage != LMI_STORAGE_F16) CHK(h->wide.reserve((size_t)n * h->d_user * 4));
    if (h->metric == LMI_METRIC_L2) CHK(h->aug_rows.reserve((size_t)n * h->d * 4));
    return 0;
}

static int add_rows_impl(lmi_index* h, const void* rows, int src16, int64_t row0, const int64_t* index, int64_t nrows, int on_device,
                         const int* pos, int64_t n_total) {
    CHK(set_dev(h));
    const size_t esz = src16 ? 2 : 4;
    const int64_t piece = ingest_piece_rows(h);
    CHK(ingest_piece_reserve(h, std::min(piece, nrows), src16, index != nullptr, on_device));   // (the first piece is the longest)
    for (int64_t off = 0; off < nrows; off += piece) {
        const int64_t n = std::min(piece, nrows - off);
        const void* raw = static_cast<const char*>(rows) + (size_t)off * h->d_user * esz;
        const long long* idx = index ? reinterpret_cast<const long long*>(index + off) : nullptr;
        if (!on_device) {
            const size_t row_bytes = (size_t)n * h->d_user * esz;
            const size_t idx_off = piece_index_offset(h, n, src16);
            HIPCHK(hipMemcpyAsync(h->stage.p, raw, row_bytes, hipMemcpyHostToDevice, h->stream));
            raw = h->stage.p;
            if (index) {
                HIPCHK(hipMemcpyAsync(h->stage.as<char>() + idx_off, index + off, (size_t)n * 8, hipMemcpyHostToDevice, h->stream));
                idx = reinterpret_cast<const long long*>(h->stage.as<char>() + idx_off);
            }
        }
        const float* src = static_cast<const float*>(raw);
        if (src16 && h->storage != LMI_STORAGE_F16) {   // halves -> the binary32 piece the kernels below were written for
            CHK(widen16_enqueue(raw, n, h->d_user, h->wide.as<float>(), h->stream));
            src = h->wide.as<float>();
        }
        if (h->metric == LMI_METRIC_L2) {  // the piece with its norm column, then ingested like any d-column piece
            augment_copy_kernel<<<cdiv((long long)n * h->d, 256), 256, 0, h->stream>>>(src, h->d_user, h->d, n, h->aug_rows.as<float>());
            HIPCHK(hipGetLastError());
            augment_norm_kernel<<<cdiv(n, 256), 256, 0, h->stream>>>(src, h->d_user, h->d, n, h->aug_rows.as<float>(), nullptr);
            HIPCHK(hipGetLastError());
            src = h->aug_rows.as<float>();
        }
        switch (stored_form(h)) {
        case FORM_FRAG16: {   // the piece -> halves -> its rows' fragments; the exactness flags and the absmax
            const long long total = (long long)n * 2 * h->KG16;
            const unsigned short* raw16 = static_cast<const unsigned short*>(raw);
            if (!src16)
                ingest16_kernel<<<cdiv(total, 256), 256, 0, h->stream>>>(src, h->d, pos, row0 + off, idx, (long long)n_total, n, h->KG16,
                                                                        frag16x16(h), h->slab16.as<uint4>(), h->xmaxbits.as<unsigned>());
            else if (half_src_vec(raw, h->d))
                ingest16_half_kernel<true><<<cdiv(total, 256), 256, 0, h->stream>>>(raw16, h->d, pos, row0 + off, idx, (long long)n_total, n, h->KG16,
                                                                                   frag16x16(h), h->slab16.as<uint4>(), h->xmaxbits.as<unsigned>());
            else
                ingest16_half_kernel<false><<<cdiv(total, 256), 256, 0, h->stream>>>(raw16, h->d, pos, row0 + off, idx, (long long)n_total, n, h->KG16,
                                                                                    frag16x16(h), h->slab16.as<uint4>(), h->xmaxbits.as<unsigned>());
            break;
        }
        case FORM_ROWMAJOR:
            scatter_rows_kernel<<<cdiv((long long)n * h->d, 256), 256, 0, h->stream>>>(src, h->d, pos, row0 + off, idx, (long long)n_total, n,
                                                                                      h->rowmajor.as<float>(), h->dp);
            break;
        case FORM_FRAG32:
            pack_scatter_kernel<<<cdiv((long long)n * h->KGs, 256), 256, 0, h->stream>>>(src, h->d, pos, row0 + off, idx, (long long)n_total, n,
                                                                                        h->KGs, h->slab.as<float4>());
            break;
        }
        HIPCHK(hipGetLastError());
        if (!on_device) HIPCHK(hipStreamSynchronize(h->stream));
    }
    return 0;
}

static int add_rows_checked(lmi_index* h, const void* rows, int src16, int64_t row0, int64_t nrows, int on_device, const char* who) {
    if (!h || !h->building) return fail("%s: call lmi_buckets_begin first", who);
    if (h->indexed_ingest) return fail("%s: this build already uses lmi_buckets_add_owned_rows", who);
    if (row0 < 0 || nrows < 0 || row0 + nrows > h->N) return fail("%s: rows [%lld,%lld) outside [0,%lld)", who, (long long)row0, (long long)(row0 + nrows), (long long)h->N);
    if (nrows == 0) return 0;
    CHK(add_rows_impl(h, rows, src16, row0, nullptr, nrows, on_device, h->pos.as<int>(), h->N));
    h->rows_added += nrows;
    return 0;
}
extern "C" LMI_API int lmi_buckets_add_rows(lmi_index* h, const float* rows, int64_t row0, int64_t nrows, int on_device) {
    return add_rows_checked(h, rows, 0, row0, nrows, on_device, "lmi_buckets_add_rows");
}
extern "C" LMI_API int lmi_buckets_add_rows_f16(lmi_index* h, const uint16_t* rows, int64_t row0, int64_t nrows, int on_device) {
    return add_rows_checked(h, rows, 1, row0, nrows, on_device, "lmi_buckets_add_rows_f16");
}

static int add_owned_rows_checked(lmi_index* h, const void* rows, int src16, const int64_t* index, int64_t nrows, int on_device, const char* who) {
    if (!h || !h->building) return fail("%s: call lmi_buckets_begin first", who);
    if (h->rows_added > 0 && !h->indexed_ingest) return fail("%s: this build already uses lmi_buckets_add_rows", who);
    if (nrows < 0 || (nrows > 0 && (!rows || !index))) return fail("%s: bad arguments", who);
    if (!on_device)
        for (int64_t i = 0; i < nrows; ++i)
            if (index[i] < 0 || index[i] >= h->N) return fail("%s: index[%lld] = %lld outside [0,%lld)", who, (long long)i, (long long)index[i], (long long)h->N);
    h->indexed_ingest = true;
    if (nrows == 0) return 0;
    CHK(add_rows_impl(h, rows, src16, 0, index, nrows, on_device, h->pos.as<int>(), h->N));
    h->rows_added += nrows;
    return 0;
}
extern "C" LMI_API int lmi_buckets_add_owned_rows(lmi_index* h, const float* rows, const int64_t* index, int64_t nrows,
                                          int on_device) {
    return add_owned_rows_checked(h, rows, 0, index, nrows, on_device, "lmi_buckets_add_owned_rows");
}
extern "C" LMI_API int lmi_buckets_add_owned_rows_f16(lmi_index* h, const uint16_t* rows, const int64_t* index, int64_t nrows,
                                              int on_device) {
    return add_owned_rows_checked(h, rows, 1, index, nrows, on_device, "lmi_buckets_add_owned_rows_f16");
}

// The prefilter's images of the whole slab: one power-of-two scale from the absmax of every stored value (holes and spare
// row-blocks hold zeros), the fp16 fragments and every bucket's norm maxima.  lmi_buckets_end, and lmi_buckets_insert when
// new rows break max|x'| < 1 under the current scale.
// the scale and every bucket's norm maxima, before they are derived again: reserved, the maxima zero
static int reset_norm_tables(lmi_index* h) {
    CHK(h->xscale.reserve(16));
    CHK(h->bnorm.reserve((size_t)h->L * 4));
    CHK(h->bdelta.reserve((size_t)h->L * 4));
    HIPCHK(hipMemsetAsync(h->bnorm.p, 0, (size_t)h->L * 4, h->stream));
    HIPCHK(hipMemsetAsync(h->bdelta.p, 0, (size_t)h->L * 4, h->stream));
    return 0;
}

static int prefilter_images(lmi_index* h) {
    // fp16 copy of the slab for the prefilter: one power-of-two scale for the whole index
    // (pass2_kernel's stages hold two k16-groups; the low-dimensional form has no stages: d = 45 is 48 wide, not 64)
    h->KG16 = kg16_for(h, h->d);
    const long long n_rows = (long long)h->n_rb_total * 32;
    CHK(h->xmaxbits.reserve(16));
    CHK(h->slab16.reserve(slab16_bytes(h)));
    HIPCHK(hipMemsetAsync(h->xmaxbits.p, 0, 16, h->stream));
    CHK(reset_norm_tables(h));
    absmax_kernel<<<h->num_cus * 8, 256, 0, h->stream>>>(h->rowmajor.as<float>(), n_rows * h->dp, h->xmaxbits.as<unsigned>());
    HIPCHK(hipGetLastError());
    make_scale_kernel<<<1, 1, 0, h->stream>>>(h->xmaxbits.as<unsigned>(), h->xscale.as<float>());
    HIPCHK(hipGetLastError());
    const long long total = n_rows * h->KG16 * 2;
    convert16_kernel<<<cdiv(total, 256), 256, 0, h->stream>>>(h->rowmajor.as<float>(), h->d, h->dp, n_rows, h->KG16,
                                                             h->xscale.as<float>(), h->slab16.as<uint4>(), frag16x16(h));
    HIPCHK(hipGetLastError());
    dim3 g(64, h->L);
    bucket_norm_kernel<<<g, 256, 0, h->stream>>>(h->rowmajor.as<float>(), h->d, h->dp, h->d_rb_start.as<int>(),
                                                h->d_nb_rows.as<int>(), h->xscale.as<float>(), h->bnorm.as<unsigned>(),
                                                h->bdelta.as<unsigned>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    h->have16 = true;
    return 0;
}

// LMI_STORAGE_F16, the images behind the fragments (lmi_buckets_end; lmi_subset on the rows it kept): the norm tables reset, the scale
// (make_scale: the caller's launch that writes xscale, and `factor` where that is another buffer), the slab times factor[0] in place
// with the S16_* flags raised in xmaxbits[1], the buckets' norms from the stored halves.  Enqueues only: the caller reads the flags.
template <class MakeScale>
static int storage16_images(lmi_index* h, const DevBuf& factor, MakeScale make_scale) {
    CHK(reset_norm_tables(h));   // (bdelta stays 0: ||x^ - x'|| = 0, the stored value IS x')
    CHK(make_scale());
    rescale16_kernel<<<h->num_cus * 8, 256, 0, h->stream>>>(h->slab16.as<uint4>(), (long long)h->n_rb_total * h->KG16 * 64, factor.as<float>(), h->xmaxbits.as<unsigned>());
    HIPCHK(hipGetLastError());
    bucket_norm16_kernel<<<dim3(64, h->L), 256, 0, h->stream>>>(h->slab16.as<uint4>(), h->d, h->KG16, frag16x16(h), h->d_rb_start.as<int>(),
                                                               h->d_nb_rows.as<int>(), h->bnorm.as<unsigned>());
    HIPCHK(hipGetLastError());
    return 0;
}

// what S16_SCALE_LOSS means, in words (lmi_buckets_end; lmi_concat, whose verdict is a fresh build's): scale = the index scale,
// maxbits = the bits of max |x|
static std::string scale_loss_reason(float scale, unsigned maxbits) {
    float mx;
    memcpy(&mx, &maxbits, 4);
    char buf[320];
    snprintf(buf, sizeof(buf), "LMI_STORAGE_F16 refused: every value is binary16-exact, but not once multiplied by the index scale %g "
                               "(max|x| = %g; a small value falls below the binary16 subnormals)", (double)scale, (double)mx);
    return buf;
}

// LMI_STORAGE_F16: the fragments were filled unscaled by lmi_buckets_add_*rows; the scale from their absmax, the slab times the scale
// in place, the buckets' norms from the stored halves -- and the verdict: the flags are read after the synchronisation, a refused
// build launches nothing more and leaves the handle without an index.
static int storage16_finish(lmi_index* h) {
    unsigned* state = h->xmaxbits.as<unsigned>();
    CHK(storage16_images(h, h->xscale, [&]() -> int {
        make_scale_kernel<<<1, 1, 0, h->stream>>>(state, h->xscale.as<float>());
        HIPCHK(hipGetLastError());
        return 0;
    }));
    unsigned st[4] = {0, 0, 0, 0};
    float sc[2] = {1.0f, 1.0f};
    HIPCHK(hipMemcpyAsync(st, state, 16, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(sc, h->xscale.p, 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (st[1] & S16_NONFINITE) return fail("lmi_buckets_end: LMI_STORAGE_F16 refused: a stored value is not finite (inf or NaN)");
    if (st[1] & S16_INEXACT) return fail("lmi_buckets_end: LMI_STORAGE_F16 refused: a stored value is not exactly representable in binary16");
    if (st[1] & S16_SCALE_LOSS) return fail("lmi_buckets_end: %s", scale_loss_reason(sc[0], st[0]).c_str());
    h->have16 = true;
    return 0;
}

extern "C" LMI_API int lmi_buckets_end(lmi_index* h) {
    if (!h || !h->building) return fail("lmi_buckets_end: call lmi_buckets_begin first");
    const int64_t expect = h->indexed_ingest ? h->owned_total : h->N;
    if (h->rows_added != expect) return fail("lmi_buckets_end: %lld of %lld rows were added", (long long)h->rows_added, (long long)expect);
    CHK(set_dev(h));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->pos.release();
    h->have16 = false;
    if (h->storage == LMI_STORAGE_F16 && h->n_rb_total > 0) {
        if (storage16_finish(h) != 0) {   // inadmissible data (or a failed call): no index; lmi_buckets_begin may be called again
            h->building = false;
            h->slab16.release();
            return -1;
        }
    } else if (h->prefilter && h->n_rb_total > 0) CHK(prefilter_images(h));
    h->building = false;
    h->built = true;
    h->layout_stamp = next_layout_stamp();
    return 0;
}

extern "C" LMI_API int lmi_bucket_sizes(lmi_index* h, int64_t* sizes) {
    if (!h || !(h->built || h->building)) return fail("lmi_bucket_sizes: no buckets");
    for (int b = 0; b < h->L; ++b) sizes[b] = h->h_nb_rows[b];
    return 0;
}

// A bucket's rows [p0, p0 + n) to the caller's `rows`, as floats or (half) as halves, enqueued on the stream.  Floats: the row-major
// copy as it lies, fragments unpacked through staging (LMI_STORAGE_F16: widened and unscaled, exact: lmi_store16.h).  Halves:
// LMI_STORAGE_F16 gives the stored halves, unscaled; the f32 forms are narrowed on the device, the flag is read after a synchronisation
// and a bucket with a value that is not binary16-exact is refused before any row reaches the caller.
static int read_rows(lmi_index* h, int bucket, int64_t p0, int64_t n, void* rows, bool half, const char* who) {
    const int du = h->d_user;  // the caller's columns (the L2 norm column is not returned)
    const StoredForm form = stored_form(h);
    const size_t out_bytes = (size_t)n * du * (half ? 2 : 4);
    if (!half && form == FORM_ROWMAJOR) {
        HIPCHK(hipMemcpy2DAsync(rows, (size_t)du * 4, h->rowmajor.as<float>() + (size_t)p0 * h->dp, (size_t)h->dp * 4, (size_t)du * 4, (size_t)n,
                                hipMemcpyDeviceToHost, h->stream));
        return 0;
    }
    CHK(h->stage.reserve(out_bytes));
    const long long pieces = n * cdiv(du, 8);
    if (!half) {
        if (form == FORM_FRAG16)
            unpack16_kernel<<<cdiv(pieces, 256), 256, 0, h->stream>>>(h->slab16.as<uint4>(), h->KG16, frag16x16(h), p0, n, du, h->xscale.as<float>(),
                                                                     h->stage.as<float>());
        else
            unpack_kernel<<<cdiv(pieces, 256), 256, 0, h->stream>>>(h->slab.as<float4>(), h->KGs, p0, n, du, h->stage.as<float>());
        HIPCHK(hipGetLastError());
    } else if (form == FORM_FRAG16) {
        unpack16_half_kernel<<<cdiv(pieces, 256), 256, 0, h->stream>>>(h->slab16.as<uint4>(), h->KG16, frag16x16(h), p0, n, du, h->xscale.as<float>(),
                                                                      h->stage.as<unsigned short>());
        HIPCHK(hipGetLastError());
    } else {
        unsigned short* out = h->stage.as<unsigned short>();
        CHK(h->rd_flag.reserve(16));
        HIPCHK(hipMemsetAsync(h->rd_flag.p, 0, 4, h->stream));
        const long long total = n * du;
        if (form == FORM_ROWMAJOR) narrow16_kernel<false><<<cdiv(total, 256), 256, 0, h->stream>>>(h->rowmajor.as<float>(), h->dp, p0, n, du, out, h->rd_flag.as<unsigned>());
        else narrow16_kernel<true><<<cdiv(total, 256), 256, 0, h->stream>>>(h->slab.as<float>(), h->KGs, p0, n, du, out, h->rd_flag.as<unsigned>());
        HIPCHK(hipGetLastError());
        unsigned bad = 0;
        HIPCHK(hipMemcpyAsync(&bad, h->rd_flag.p, 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        if (bad) return fail("%s: a value of bucket %d is not exactly representable in binary16 (or not finite); nothing was returned -- read it with lmi_bucket_read", who, bucket);
    }
    HIPCHK(hipMemcpyAsync(rows, h->stage.p, out_bytes, hipMemcpyDeviceToHost, h->stream));
    return 0;
}

// lmi_bucket_read / lmi_bucket_read_f16 (half: the rows as halves; `who`: the entry point, for the messages).  Reads only.
static int bucket_read_impl(lmi_index* h, int bucket, void* rows, bool half, uint32_t* ids, const char* who) {
    if (!h || !h->built) return fail("%s: the bucket index is not built", who);
    if (bucket < 0 || bucket >= h->L) return fail("%s: bucket %d outside [0,%d)", who, bucket, h->L);
    const int64_t n = h->h_nb_rows[bucket];
    if (n == 0) return 0;
    CHK(set_dev(h));
    const int64_t p0 = (int64_t)h->h_rb_start[bucket] * 32;
    if (rows) CHK(read_rows(h, bucket, p0, n, rows, half, who));
    if (ids) HIPCHK(hipMemcpyAsync(ids, h->ids_slab.as<uint32_t>() + p0, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}
extern "C" LMI_API int lmi_bucket_read(lmi_index* h, int bucket, float* rows, uint32_t* ids) {
    return bucket_read_impl(h, bucket, rows, false, ids, "lmi_bucket_read");
}
extern "C" LMI_API int lmi_bucket_read_f16(lmi_index* h, int bucket, uint16_t* rows, uint32_t* ids) {
    return bucket_read_impl(h, bucket, rows, true, ids, "lmi_bucket_read_f16");
}
