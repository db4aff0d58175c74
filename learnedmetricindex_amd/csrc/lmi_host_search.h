// lmi_host_search.h -- the search calls of the ABI: argument checks and output staging around mlp_enqueue / nav_enqueue /
// scan_enqueue (lmi_scan_topk, lmi_search, lmi_search_tree, lmi_knn_ip), the device-side copies and lmi_pipeline_submit.
#pragma once
#include "lmi_host_model.h"
#include "lmi_host_scan.h"

static int check_scan_args(lmi_index* h, int nq, int nb, int k, int* kout, const char* who = "lmi_scan_topk") {
    if (!h->built) return fail("%s: the bucket index is not built (lmi_buckets_begin/add_rows/end)", who);
    if (nq < 0 || nb < 1) return fail("%s: bad nq/n_buckets", who);
    if (nb > 1024) return fail("%s: n_buckets %d exceeds 1024 (the rank merge keeps 16 four-bit cursors per lane)", who, nb);
    if (k < 1 || k > LMI_MAX_K) return fail("%s: k %d outside [1,%d]", who, k, LMI_MAX_K);
    *kout = nb == 1 ? KPB : k;  // LearnedIndex.py:122-124: a single rank is returned unmerged
    if ((long long)nb * KPB < *kout) return fail("%s: k %d exceeds n_buckets*10 candidates", who, k);
    if ((long long)nq * nb >= (1ll << 31)) return fail("%s: nq*n_buckets too large", who);
    return 0;
}

// Where a search call's kernels write dists / ids / keys [nq][kout]: the caller's device buffers, or the handle's staging buffers
// for a host-pointer call, which copy_back returns to the caller (dists, ids, keys, then what else the call hands back).
struct OutStage {
    float* d;
    uint32_t* id;
    uint32_t* key;
    size_t bytes;   // of one array
};
static int out_stage(lmi_index* h, int nq, int kout, float* dists, uint32_t* ids, uint32_t* keys, int on_device, OutStage& o) {
    o.d = dists; o.id = ids; o.key = keys;
    o.bytes = (size_t)nq * kout * 4;
    if (on_device) return 0;
    CHK(h->out_d.reserve(o.bytes));
    CHK(h->out_id.reserve(o.bytes));
    o.d = h->out_d.as<float>();
    o.id = h->out_id.as<uint32_t>();
    if (keys) { CHK(h->out_key.reserve(o.bytes)); o.key = h->out_key.as<uint32_t>(); }
    return 0;
}

// The three search calls take their queries as binary32 or (q16; the *_f16 entry points) as halves: a half array is uploaded as it is
// -- half the bytes -- and widened on the device into the handle's q_nav / q_srch (input_ptr16; with on_device from the caller's
// memory, which is only read); from there on the call is the binary32 call on the widened values.
static int scan_topk_impl(lmi_index* h, const void* queries_search, int q16, int nq, const int32_t* bucket_order,
                          int nb, int k, float* dists, uint32_t* ids, uint32_t* keys, int on_device) {
    if (!h) return fail("%s: NULL handle", q16 ? "lmi_scan_topk_f16" : "lmi_scan_topk");
    int kout = 0;
    CHK(check_scan_args(h, nq, nb, k, &kout, q16 ? "lmi_scan_topk_f16" : "lmi_scan_topk"));
    if (nq == 0) return 0;
    CHK(set_dev(h));
    const void* d_qs = nullptr;
    const void* d_order = nullptr;
    if (q16) CHK(input_ptr16(h, queries_search, nq, h->d_user, on_device, h->q16_srch, h->q_srch, &d_qs));
    else CHK(input_ptr(h, queries_search, (size_t)nq * h->d_user * 4, on_device, h->q_srch, &d_qs));
    CHK(input_ptr(h, bucket_order, (size_t)nq * nb * 4, on_device, h->order, &d_order));
    OutStage o;
    CHK(out_stage(h, nq, kout, dists, ids, keys, on_device, o));
    begin_call(h);
    CHK(record(h, 1));
    CHK(scan_enqueue(h, static_cast<const float*>(d_qs), nq, static_cast<const int*>(d_order), nb, kout, 0, o.d, o.id, o.key));
    if (!on_device) CHK(copy_back(h, {{dists, o.d, o.bytes}, {ids, o.id, o.bytes}, {keys, o.key, o.bytes}}));
    return 0;
}

extern "C" LMI_API int lmi_scan_topk(lmi_index* h, const float* queries_search, int nq, const int32_t* bucket_order,
                             int nb, int k, float* dists, uint32_t* ids, uint32_t* keys, int on_device) {
    return scan_topk_impl(h, queries_search, 0, nq, bucket_order, nb, k, dists, ids, keys, on_device);
}
extern "C" LMI_API int lmi_scan_topk_f16(lmi_index* h, const uint16_t* queries_search, int nq, const int32_t* bucket_order,
                                 int nb, int k, float* dists, uint32_t* ids, uint32_t* keys, int on_device) {
    return scan_topk_impl(h, queries_search, 1, nq, bucket_order, nb, k, dists, ids, keys, on_device);
}

static int search_impl(lmi_index* h, const void* queries_nav, const void* queries_search, int q16, int nq, int nb,
                       int k, float* dists, uint32_t* ids, uint32_t* keys, int32_t* bucket_order, int on_device) {
    const char* who = q16 ? "lmi_search_f16" : "lmi_search";
    if (!h) return fail("%s: NULL handle", who);
    int kout = 0;
    CHK(check_scan_args(h, nq, nb, k, &kout, q16 ? "lmi_scan_topk_f16" : "lmi_scan_topk"));
    if (h->root().n_layers == 0) return fail("%s: no MLP set (lmi_set_mlp)", who);
    if (h->root().dims.back() != h->L) return fail("%s: MLP has %d classes, index has %d buckets", who, h->root().dims.back(), h->L);
    if (nq == 0) return 0;
    CHK(set_dev(h));
    const void* d_qn = nullptr;
    const void* d_qs = nullptr;
    if (q16) CHK(input_ptr16(h, queries_nav, nq, h->root().dims[0], on_device, h->q16_nav, h->q_nav, &d_qn));
    else CHK(input_ptr(h, queries_nav, (size_t)nq * h->root().dims[0] * 4, on_device, h->q_nav, &d_qn));
    if (queries_search == queries_nav && h->root().dims[0] == h->d_user) d_qs = d_qn;
    else if (q16) CHK(input_ptr16(h, queries_search, nq, h->d_user, on_device, h->q16_srch, h->q_srch, &d_qs));
    else CHK(input_ptr(h, queries_search, (size_t)nq * h->d_user * 4, on_device, h->q_srch, &d_qs));
    int* d_order = bucket_order;
    if (!on_device || !bucket_order) { CHK(h->order.reserve((size_t)nq * nb * 4)); d_order = h->order.as<int>(); }
    OutStage o;
    CHK(out_stage(h, nq, kout, dists, ids, keys, on_device, o));
    begin_call(h);
    CHK(record(h, 0));
    CHK(mlp_enqueue(h, static_cast<const float*>(d_qn), nq, nb, d_order, nullptr));
    CHK(record(h, 1));
    CHK(scan_enqueue(h, static_cast<const float*>(d_qs), nq, d_order, nb, kout, 0, o.d, o.id, o.key));
    if (!on_device) CHK(copy_back(h, {{dists, o.d, o.bytes}, {ids, o.id, o.bytes}, {keys, o.key, o.bytes}, {bucket_order, d_order, (size_t)nq * nb * 4}}));
    return 0;
}

extern "C" LMI_API int lmi_search(lmi_index* h, const float* queries_nav, const float* queries_search, int nq, int nb,
                          int k, float* dists, uint32_t* ids, uint32_t* keys, int32_t* bucket_order, int on_device) {
    return search_impl(h, queries_nav, queries_search, 0, nq, nb, k, dists, ids, keys, bucket_order, on_device);
}
extern "C" LMI_API int lmi_search_f16(lmi_index* h, const uint16_t* queries_nav, const uint16_t* queries_search, int nq, int nb,
                              int k, float* dists, uint32_t* ids, uint32_t* keys, int32_t* bucket_order, int on_device) {
    return search_impl(h, queries_nav, queries_search, 1, nq, nb, k, dists, ids, keys, bucket_order, on_device);
}

// LearnedIndex.search for a multi-level index in ONE call (LearnedIndex.py:216-325 the walk, :328-373 the bucket scans): lmi_nav_order +
// lmi_scan_topk without the host in between.  Host buffers: the scan vectors' upload (30 MB at 10 000 x 768: 1.2 ms from pageable memory)
// goes over the library's side stream WHILE the walk runs (0.4-1 ms); the walk's bucket order never leaves the device unless asked for.
// q16: the halves of the scan vectors take the same side-stream upload (15 MB there) and are widened into q_srch behind the join.
static int search_tree_impl(lmi_index* h, const void* queries_nav, const void* queries_search, int q16, int nq, int nb, int k,
                            float* dists, uint32_t* ids, uint32_t* keys, int32_t* slab_ids, int32_t* entries, int on_device) {
    const char* who = q16 ? "lmi_search_tree_f16" : "lmi_search_tree";
    if (!h) return fail("%s: NULL handle", who);
    int kout = 0;
    CHK(check_scan_args(h, nq, nb, k, &kout, q16 ? "lmi_scan_topk_f16" : "lmi_scan_topk"));
    if (nq == 0) return 0;
    CHK(nav_check(h, nq, nb, who));
    const void* d_qn = nullptr;
    const void* d_qs = queries_search;
    if (q16) CHK(input_ptr16(h, queries_nav, nq, h->root().dims[0], on_device, h->q16_nav, h->q_nav, &d_qn));
    else CHK(input_ptr(h, queries_nav, (size_t)nq * h->root().dims[0] * 4, on_device, h->q_nav, &d_qn));
    const bool same = queries_search == queries_nav && h->root().dims[0] == h->d_user;
    if (same) d_qs = d_qn;
    CHK(h->nav_slab.reserve((size_t)nq * nb * 4));
    CHK(h->nav_ent.reserve((size_t)nq * nb * 4));
    int* d_slab = (on_device && slab_ids) ? slab_ids : h->nav_slab.as<int>();
    int* d_ent = (on_device && entries) ? entries : h->nav_ent.as<int>();
    OutStage o;
    CHK(out_stage(h, nq, kout, dists, ids, keys, on_device, o));
    // q_srch is written from the side stream below.  Its last reader is the previous call's scan: a host-pointer call ended
    // synchronised, but an on_device *_f16 call widened into q_srch and its scan may still be reading it -- then the side stream
    // first waits for everything enqueued so far (here, before the walk is enqueued, so the upload still runs beside the walk)
    if (!on_device && !same && !q16 && h->q_srch_async) {
        CHK(side_fork(h));
        h->q_srch_async = false;
    }
    if ((!on_device || q16) && !same) CHK(h->q_srch.reserve((size_t)nq * h->d_user * 4));
    if (q16 && !on_device && !same) CHK(h->q16_srch.reserve((size_t)nq * h->d_user * 2));
    begin_call(h);
    CHK(record(h, 0));
    CHK(nav_enqueue(h, static_cast<const float*>(d_qn), nq, nb, d_slab, d_ent));
    CHK(record(h, 1));
    CHK(stamp_end(h, ST_MLP1));
    if (!on_device && !same) {
        // the scan vectors: uploaded beside the walk (the copy's host side returns when the bytes are staged; the stream waits for its event)
        CHK(side_ensure(h));   // (no fork here: see q_srch_async above; q16_srch's last reader was a host-pointer call's widening, which ended synchronised)
        if (q16) HIPCHK(hipMemcpyAsync(h->q16_srch.p, queries_search, (size_t)nq * h->d_user * 2, hipMemcpyHostToDevice, h->side));
        else HIPCHK(hipMemcpyAsync(h->q_srch.p, queries_search, (size_t)nq * h->d_user * 4, hipMemcpyHostToDevice, h->side));
        HIPCHK(hipEventRecord(h->side_join, h->side));
        HIPCHK(hipStreamWaitEvent(h->stream, h->side_join, 0));
        if (q16) CHK(widen16_enqueue(h->q16_srch.p, nq, h->d_user, h->q_srch.as<float>(), h->stream));
        d_qs = h->q_srch.p;
    } else if (q16 && !same) {   // device halves: widened into the handle's buffer
        h->q_srch_async = true;
        CHK(widen16_enqueue(queries_search, nq, h->d_user, h->q_srch.as<float>(), h->stream));
        d_qs = h->q_srch.p;
    }
    CHK(scan_enqueue(h, static_cast<const float*>(d_qs), nq, d_slab, nb, kout, 0, o.d, o.id, o.key));
    if (!on_device) CHK(copy_back(h, {{dists, o.d, o.bytes}, {ids, o.id, o.bytes}, {keys, o.key, o.bytes},
                                      {slab_ids, d_slab, (size_t)nq * nb * 4}, {entries, d_ent, (size_t)nq * nb * 4}}));
    return 0;
}

extern "C" LMI_API int lmi_search_tree(lmi_index* h, const float* queries_nav, const float* queries_search, int nq, int nb, int k,
                               float* dists, uint32_t* ids, uint32_t* keys, int32_t* slab_ids, int32_t* entries, int on_device) {
    return search_tree_impl(h, queries_nav, queries_search, 0, nq, nb, k, dists, ids, keys, slab_ids, entries, on_device);
}
extern "C" LMI_API int lmi_search_tree_f16(lmi_index* h, const uint16_t* queries_nav, const uint16_t* queries_search, int nq, int nb, int k,
                                   float* dists, uint32_t* ids, uint32_t* keys, int32_t* slab_ids, int32_t* entries, int on_device) {
    return search_tree_impl(h, queries_nav, queries_search, 1, nq, nb, k, dists, ids, keys, slab_ids, entries, on_device);
}

extern "C" LMI_API int lmi_knn_ip(int device, const float* xq, int64_t nq, const float* xb, int64_t nb, int d, int k,
                          float* D, int64_t* I) {
    if (k < 1 || k > KPB) return fail("lmi_knn_ip: k %d outside [1,%d]", k, KPB);
    if (nq < 0 || nb < 0 || d < 1) return fail("lmi_knn_ip: bad sizes");
    if (nq >= (1ll << 31)) return fail("lmi_knn_ip: nq too large");
    for (int64_t i = 0; i < nq * k; ++i) { D[i] = -FLT_MAX; I[i] = -1; }
    if (nq == 0 || nb == 0) return 0;
    lmi_index* h = nullptr;
    CHK(lmi_create(device, &h));
    int rc = 0;
    std::vector<int64_t> labels((size_t)nb, 0);
    std::vector<int32_t> order((size_t)nq, 0);
    std::vector<float> dd((size_t)nq * KPB);
    std::vector<uint32_t> ii((size_t)nq * KPB);
    do {
        if ((rc = lmi_buckets_begin(h, nb, d, 1, labels.data(), nullptr, nullptr))) break;
        if ((rc = lmi_buckets_add_rows(h, xb, 0, nb, 0))) break;
        if ((rc = lmi_buckets_end(h))) break;
        if ((rc = hipSetDevice(device) == hipSuccess ? 0 : fail("hipSetDevice"))) break;
        const void *d_qs, *d_order;
        if ((rc = input_ptr(h, xq, (size_t)nq * d * 4, 0, h->q_srch, &d_qs))) break;
        if ((rc = input_ptr(h, order.data(), (size_t)nq * 4, 0, h->order, &d_order))) break;
        if ((rc = h->out_d.reserve((size_t)nq * KPB * 4))) break;
        if ((rc = h->out_id.reserve((size_t)nq * KPB * 4))) break;
        if ((rc = scan_enqueue(h, static_cast<const float*>(d_qs), (int)nq, static_cast<const int*>(d_order), 1, KPB, 1,
                               h->out_d.as<float>(), h->out_id.as<uint32_t>(), nullptr))) break;
        if (hipMemcpy(dd.data(), h->out_d.p, dd.size() * 4, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(ii.data(), h->out_id.p, ii.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) {
            rc = fail("lmi_knn_ip: result copy failed");
            break;
        }
        for (int64_t q = 0; q < nq; ++q)
            for (int j = 0; j < k; ++j) {
                D[q * k + j] = dd[q * KPB + j];
                I[q * k + j] = ii[q * KPB + j] == NOROW ? -1 : (int64_t)ii[q * KPB + j];
            }
    } while (0);
    std::string keep = g_err;
    lmi_destroy(h);
    if (rc) g_err = keep;
    return rc;
}

extern "C" LMI_API int lmi_copy_out(lmi_index* h, void* dst, const void* src, int64_t bytes) {
    if (!h) return fail("lmi_copy_out: NULL handle");
    if (bytes < 0 || (bytes > 0 && (!dst || !src))) return fail("lmi_copy_out: bad arguments");
    if ((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src)) & 15) return fail("lmi_copy_out: pointers must be 16-byte aligned");
    if (bytes == 0) return 0;
    CHK(set_dev(h));
    const int blocks = (int)std::min<long long>(h->num_cus * 2, cdiv(cdiv(bytes, 16), 256));
    copy_bytes_kernel<<<std::max(1, blocks), 256, 0, h->stream>>>(static_cast<const unsigned char*>(src), static_cast<unsigned char*>(dst), bytes);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" LMI_API int lmi_copy_out_many(lmi_index* h, int n, void* const* dst, const void* const* src, const int64_t* bytes) {
    if (!h) return fail("lmi_copy_out_many: NULL handle");
    if (n < 0 || n > 4 || (n > 0 && (!dst || !src || !bytes))) return fail("lmi_copy_out_many: bad arguments (1..4 ranges)");
    CopyRanges C;
    long long most = 0;
    int used = 0;
    for (int i = 0; i < n; ++i) {
        if (bytes[i] < 0 || (bytes[i] > 0 && (!dst[i] || !src[i]))) return fail("lmi_copy_out_many: bad range %d", i);
        if ((reinterpret_cast<uintptr_t>(dst[i]) | reinterpret_cast<uintptr_t>(src[i])) & 15) return fail("lmi_copy_out_many: pointers must be 16-byte aligned");
        if (bytes[i] == 0) continue;
        C.src[used] = static_cast<const unsigned char*>(src[i]);
        C.dst[used] = static_cast<unsigned char*>(dst[i]);
        C.bytes[used] = bytes[i];
        most = std::max<long long>(most, bytes[i]);
        ++used;
    }
    if (used == 0) return 0;
    CHK(set_dev(h));
    const int bx = (int)std::max<long long>(1, std::min<long long>(h->num_cus, cdiv(cdiv(most, 16), 256)));
    copy_ranges_kernel<<<dim3(bx, used), 256, 0, h->stream>>>(C);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" LMI_API int lmi_pipeline_submit(lmi_index* h, void* s_in_, void* s_nav_, void* s_run_, void* ev_in_, void* ev_nav_, void* ev_out_,
                                          const float* qn_host, const float* qs_host, float* qn_dev, float* qs_dev, int nq, int nb, int k,
                                          float* dists_out, uint32_t* ids_out, int32_t* bo_dev, int32_t* bo_host, int overlap_nav) {
    if (!h) return fail("lmi_pipeline_submit: NULL handle");
    if (!s_in_ || !s_run_ || !ev_in_ || !ev_out_ || !qn_host || !qn_dev || !dists_out || !ids_out || !bo_dev) return fail("lmi_pipeline_submit: NULL argument");
    if (overlap_nav && (!s_nav_ || !ev_nav_)) return fail("lmi_pipeline_submit: overlap_nav needs a navigation stream and event");
    if ((qs_host == nullptr) != (qs_dev == nullptr)) return fail("lmi_pipeline_submit: qs_host and qs_dev go together");
    if (nq < 1 || h->root().n_layers == 0 || !h->built) return fail("lmi_pipeline_submit: empty batch, no MLP or no bucket index");
    CHK(set_dev(h));
    hipStream_t s_in = static_cast<hipStream_t>(s_in_), s_nav = static_cast<hipStream_t>(s_nav_), s_run = static_cast<hipStream_t>(s_run_);
    hipEvent_t ev_in = static_cast<hipEvent_t>(ev_in_), ev_nav = static_cast<hipEvent_t>(ev_nav_), ev_out = static_cast<hipEvent_t>(ev_out_);
    HIPCHK(hipMemcpyAsync(qn_dev, qn_host, (size_t)nq * h->root().dims[0] * 4, hipMemcpyHostToDevice, s_in));
    if (qs_host) HIPCHK(hipMemcpyAsync(qs_dev, qs_host, (size_t)nq * h->d_user * 4, hipMemcpyHostToDevice, s_in));
    HIPCHK(hipEventRecord(ev_in, s_in));
    const float* q_scan = qs_dev ? qs_dev : qn_dev;
    if (overlap_nav) {
        HIPCHK(hipStreamWaitEvent(s_nav, ev_in, 0));
        h->stream = s_nav;
        int rc = lmi_mlp_topk(h, qn_dev, nq, nb, bo_dev, nullptr, 1);
        h->stream = s_run;
        CHK(rc);
        HIPCHK(hipEventRecord(ev_nav, s_nav));
        HIPCHK(hipStreamWaitEvent(s_run, ev_nav, 0));
        CHK(lmi_scan_topk(h, q_scan, nq, bo_dev, nb, k, dists_out, ids_out, nullptr, 1));
    } else {
        h->stream = s_run;
        HIPCHK(hipStreamWaitEvent(s_run, ev_in, 0));
        CHK(lmi_search(h, qn_dev, q_scan, nq, nb, k, dists_out, ids_out, nullptr, bo_dev, 1));
    }
    if (bo_host) CHK(lmi_copy_out(h, bo_host, bo_dev, (int64_t)nq * nb * 4));
    HIPCHK(hipEventRecord(ev_out, s_run));
    return 0;
}
