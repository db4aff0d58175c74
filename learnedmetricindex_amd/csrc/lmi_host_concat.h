// lmi_host_concat.h -- lmi_concat: a new, independent index that holds the objects of several built indexes over the same partition,
// and the plan words (kernels: lmi_concat.h; the arithmetic: lmi_concat_plan.h; include/lmi_hip.h states the contract).
#pragma once
#include "lmi_host_call.h"
#include "lmi_host_subset.h"
#include "lmi_concat.h"
#include "lmi_concat_plan.h"

// ------------------------------------------------------------------------------------------------
// No reference counterpart (the reference concatenates its DataFrames and rebuilds).  lmi_subset is "same labels, fewer objects",
// lmi_regroup "same objects, new labels"; this is "same labels, the objects of several indexes".  The new handle is what lmi_create +
// parts[0]'s settings + lmi_buckets_begin / add_rows / end over "parts[0]'s objects in the order it holds them, then parts[1]'s, ..."
// would be: the host lays the new index out from the sums of the parts' counts (lmi_concat_plan.h, begin_layout), one kernel writes
// per row of the new slab where it comes from, one gather moves the stored image with the ids alongside, and what a build derives
// from the rows is derived from the new handle's own rows.  The parts are only read.
// The call's maps: 8 bytes per slab row of the new index (the source map) and three small tables per (part, bucket); all of them are
// freed before the call returns.
namespace {
thread_local int64_t g_concat_last[LMI_CONCAT_PLAN_COUNT] = {};

const char* metric_name(int m) { return m == LMI_METRIC_L2 ? "LMI_METRIC_L2" : "LMI_METRIC_IP"; }
const char* storage_name(int s) { return s == LMI_STORAGE_F16 ? "LMI_STORAGE_F16" : "LMI_STORAGE_F32"; }

// the refusals of lmi_concat_plan.h in words
int concat_refusal(const lmi_concat_plan::Verdict& v, int L) {
    namespace cp = lmi_concat_plan;
    const long long val = (long long)v.value, want = (long long)v.want;
    switch (v.problem) {
    case cp::OK: return 0;
    case cp::BAD_N_PARTS: return fail("lmi_concat: n_parts = %lld outside [1, %d]", val, cp::MAX_PARTS);
    case cp::DEVICE: return fail("lmi_concat: parts[%d] is on device %lld, parts[0] on device %lld", v.part, val, want);
    case cp::DIMS: return fail("lmi_concat: parts[%d] differs from parts[0] in d: %lld, not %lld", v.part, val, want);
    case cp::BUCKETS: return fail("lmi_concat: parts[%d] differs from parts[0] in L: %lld buckets, not %lld", v.part, val, want);
    case cp::METRIC:
        return fail("lmi_concat: parts[%d] differs from parts[0] in the metric: %s, not %s", v.part, metric_name((int)val), metric_name((int)want));
    case cp::STORAGE:
        return fail("lmi_concat: parts[%d] differs from parts[0] in the storage: %s, not %s", v.part, storage_name((int)val), storage_name((int)want));
    case cp::PREFILTER:
        return fail("lmi_concat: parts[%d] differs from parts[0] in the prefilter: %s, not %s (the index is stored differently)", v.part,
                    val ? "on" : "off", want ? "on" : "off");
    case cp::OWNED:
        if (val != want)
            return fail("lmi_concat: parts[%d] differs from parts[0] in the owned mask: it has %s, parts[0] has %s", v.part, val ? "one" : "none",
                        want ? "one" : "none");
        return fail("lmi_concat: parts[%d] differs from parts[0] in the owned mask at bucket %lld", v.part, (long long)v.at);
    case cp::N_PAST_LIMIT: return fail("lmi_concat: the parts hold %lld objects together: N too large for 32-bit positions", val);
    case cp::BUCKET_PAST_LIMIT:
        return fail("lmi_concat: bucket %lld would hold %lld rows, past the 32-bit positions of the slab", (long long)v.at, val);
    case cp::TOTAL_PAST_LIMIT:
        return fail("lmi_concat: the layout would span %lld row-blocks, past the 32-bit positions of the slab (at most %lld)", val,
                    (long long)lmi_layout::max_slab_rb(L));
    }
    return fail("internal: unknown verdict (%s:%d)", __FILE__, __LINE__);
}
}  // namespace

// everything of lmi_concat behind the checks: fills the fresh handle c from the parts (their streams are idle; c runs on the NULL stream)
static int concat_fill(lmi_index* const* parts, int n_parts, lmi_index* c, const lmi_concat_plan::Plan& P, int64_t* n_total) {
    const lmi_index* h = parts[0];
    const int L = h->L;
    hipStream_t st = c->stream;
    // ---- parts[0]'s settings, models and tree: L and the buckets' meaning are the same, so its tables are valid ----
    CHK(inherit_handle(h, c, true));
    // ---- 1: the layout of a fresh build of all the parts' objects ----
    CHK(begin_layout(c, P.N, h->d_user, L, P.counts.data(), P.any.data(), h->h_owned.empty() ? nullptr : h->h_owned.data(), "lmi_concat"));
    if (c->d != h->d || c->dp != h->dp || c->KGs != h->KGs || (c->prefilter && c->storage == LMI_STORAGE_F16 && (c->KG16 != h->KG16 || frag16x16(c) != frag16x16(h))))
        return fail("internal: the new handle's images are shaped differently from the parts' (%s:%d)", __FILE__, __LINE__);
    if (c->n_rb_total != P.n_rb_total || c->h_rb_start != P.rb_start)
        return fail("internal: the new handle's layout is not the plan's (%s:%d)", __FILE__, __LINE__);
    const int64_t new_rows = c->n_rb_total * 32;
    const StoredForm form = stored_form(c);
    HIPCHK(hipMemsetAsync(c->ids_slab.p, 0, (size_t)std::max<int64_t>(c->n_rb_total, 1) * 32 * 4, st));
    CallScratch mem("lmi_concat");
    std::vector<ConcatPart> table((size_t)n_parts);
    std::vector<int> tabs((size_t)3 * n_parts * L);   // first_row | n_rows | offset, [n_parts][L] each (alive until the stream has taken them)
    ConcatPart* d_parts = nullptr;
    if (P.rows > 0) {
        // ---- 2: the table of the parts and, per row of the NEW slab, the part and the part's slab row it comes from ----
        for (int t = 0; t < n_parts; ++t) {
            const lmi_index* p = parts[t];
            const bool has_rows = p->owned_total > 0;
            const DevBuf& image = form == FORM_FRAG16 ? p->slab16 : form == FORM_ROWMAJOR ? p->rowmajor : p->slab;
            table[(size_t)t] = ConcatPart{image.p, p->ids_slab.as<uint32_t>(), form == FORM_FRAG16 && has_rows ? p->xmaxbits.as<unsigned>() : nullptr,
                                          form == FORM_FRAG16 && has_rows ? p->xscale.as<float>() : nullptr, 1.0f, 0};
            for (int b = 0; b < L; ++b) {
                tabs[((size_t)0 * n_parts + t) * L + b] = p->h_rb_start[(size_t)b] * 32;
                tabs[((size_t)1 * n_parts + t) * L + b] = p->h_nb_rows[(size_t)b];
                tabs[((size_t)2 * n_parts + t) * L + b] = P.offset(t, b);
            }
        }
        int* d_tabs = nullptr;
        int2* srcmap = nullptr;
        CHK(mem.alloc(&d_parts, table.size() * sizeof(ConcatPart), "table of the parts"));
        CHK(mem.alloc(&d_tabs, tabs.size() * 4, "per-part bucket tables"));
        CHK(mem.alloc(&srcmap, (size_t)new_rows * 8, "source map"));
        HIPCHK(hipMemcpyAsync(d_parts, table.data(), table.size() * sizeof(ConcatPart), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_tabs, tabs.data(), tabs.size() * 4, hipMemcpyHostToDevice, st));
        const int max_n = *std::max_element(P.counts.begin(), P.counts.end());
        const size_t plane = (size_t)n_parts * L;
        concat_srcmap_kernel<<<dim3(std::max(1, std::min(64, cdiv(max_n, 256))), L), 256, 0, st>>>(
            d_tabs, d_tabs + plane, d_tabs + 2 * plane, n_parts, L, c->d_rb_start.as<int>(), c->d_nb_rows.as<int>(), srcmap);
        HIPCHK(hipGetLastError());
        // ---- 3: the gather of the stored image, the ids alongside ----
        switch (form) {
        case FORM_FRAG16: {
            // every part stores x * s_t under its own scale; the result's scale from the largest of the parts' maxima, part t's halves
            // times the power of two s_out / s_t <= 1 on the way.  Going down in exponent can lose bits: the gather raises S16_SCALE_LOSS
            CHK(c->xscale.reserve(16));
            CHK(c->mut_stage.reserve(16));
            concat_scale16_kernel<<<1, 1, 0, st>>>(d_parts, n_parts, c->xmaxbits.as<unsigned>(), c->xscale.as<float>(), c->mut_stage.as<float>());
            HIPCHK(hipGetLastError());
            const long long pieces = c->n_rb_total * c->KG16 * 64;
            concat_gather_frag16_kernel<<<gather_blocks(c, pieces), 256, 0, st>>>(d_parts, srcmap, c->n_rb_total, c->KG16, frag16x16(c),
                                                                                   c->slab16.as<uint4>(), c->ids_slab.as<uint32_t>(),
                                                                                   c->xmaxbits.as<unsigned>());
            break;
        }
        case FORM_ROWMAJOR: {
            const long long pieces = new_rows * (c->dp / 4);
            concat_gather_rows_kernel<<<gather_blocks(c, pieces), 256, 0, st>>>(d_parts, srcmap, new_rows, c->dp / 4, c->rowmajor.as<float4>(),
                                                                                 c->ids_slab.as<uint32_t>());
            break;
        }
        case FORM_FRAG32: {
            const long long pieces = c->n_rb_total * c->KGs * 64;
            concat_gather_frag32_kernel<<<gather_blocks(c, pieces), 256, 0, st>>>(d_parts, srcmap, c->n_rb_total, c->KGs, c->slab.as<float4>(),
                                                                                   c->ids_slab.as<uint32_t>());
            break;
        }
        }
        HIPCHK(hipGetLastError());
    }
    // ---- 4: what lmi_buckets_end derives from the rows, from the new handle's own ----
    c->rows_added = c->N;
    c->have16 = false;
    unsigned st16[2] = {0u, 0u};   // LMI_STORAGE_F16: [0] the bits of max |x|, [1] the S16_* flags the gather raised
    float sc[2] = {1.0f, 1.0f};
    if (form == FORM_FRAG16 && c->n_rb_total > 0) {
        // the scale is made and the halves are under it already (2, 3): the factor is 1 and the slab stays as gathered
        CHK(storage16_images(c, c->mut_stage, []() -> int { return 0; }));
        HIPCHK(hipMemcpyAsync(st16, c->xmaxbits.p, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(sc, c->xscale.p, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(table.data(), d_parts, table.size() * sizeof(ConcatPart), hipMemcpyDeviceToHost, st));   // (the ratios)
        c->have16 = true;
    } else if (c->prefilter && c->n_rb_total > 0) {
        CHK(prefilter_images(c));   // its own absmax, scale, fp16 fragments and norms
    }
    HIPCHK(hipStreamSynchronize(st));   // (the maps free themselves behind it)
    // the verdict a fresh build of the same rows reaches: x * s_out must be a half
    if (st16[1] & S16_SCALE_LOSS) return fail("%s", scale_loss_reason(sc[0], st16[0]).c_str());
    if (st16[1]) return fail("internal: the gather of the halves raised the flags %u (%s:%d)", st16[1], __FILE__, __LINE__);
    c->mut_stage.release();
    c->building = false;
    c->built = true;
    c->layout_stamp = next_layout_stamp();   // its own layout: no filter of a part fits it
    if (n_total) *n_total = P.rows;
    int64_t rescaled = 0;
    for (const ConcatPart& p : table) rescaled += p.ratio != 1.0f;
    g_concat_last[LMI_CONCAT_PLAN_PARTS] = n_parts;
    g_concat_last[LMI_CONCAT_PLAN_ROWS] = P.rows;
    g_concat_last[LMI_CONCAT_PLAN_SLAB_ROWS] = new_rows;
    g_concat_last[LMI_CONCAT_PLAN_MAP_BYTES] = mem.total;
    g_concat_last[LMI_CONCAT_PLAN_RESCALED_PARTS] = rescaled;
    return 0;
}

extern "C" LMI_API int lmi_debug_concat_plan(int64_t* out, int n) {
    if (!out || n < 0) return fail("lmi_debug_concat_plan: NULL argument");
    for (int i = 0; i < std::min(n, (int)LMI_CONCAT_PLAN_COUNT); ++i) out[i] = g_concat_last[i];
    return 0;
}

extern "C" LMI_API int lmi_concat(lmi_index* const* parts, int n_parts, lmi_index** out, int64_t* n_total) {
    namespace cp = lmi_concat_plan;
    for (int64_t& w : g_concat_last) w = 0;
    if (!out) return fail("lmi_concat: out is NULL");
    *out = nullptr;
    if (n_total) *n_total = 0;
    if (!parts) return fail("lmi_concat: parts is NULL");
    if (!cp::n_parts_ok(n_parts)) return concat_refusal(cp::Verdict{cp::BAD_N_PARTS, 0, 0, n_parts, 0}, 0);
    std::vector<cp::Shape> shapes((size_t)n_parts);
    std::vector<std::vector<int>> rows((size_t)n_parts);
    std::vector<std::vector<unsigned char>> any((size_t)n_parts);
    std::vector<int64_t> N((size_t)n_parts);
    for (int t = 0; t < n_parts; ++t) {
        const lmi_index* p = parts[t];
        if (!p) return fail("lmi_concat: parts[%d] is NULL", t);
        if (p->building) return fail("lmi_concat: parts[%d] is being built (lmi_buckets_end has not run)", t);
        if (!p->built) return fail("lmi_concat: parts[%d] is not built (lmi_buckets_end has not run)", t);
        shapes[(size_t)t] = cp::Shape{p->device, p->d_user, p->L, p->metric, p->storage, p->prefilter, p->h_owned};
        rows[(size_t)t] = p->h_nb_rows;
        any[(size_t)t] = p->h_any;
        N[(size_t)t] = p->N;
    }
    CHK(concat_refusal(cp::compatible(shapes), parts[0]->L));
    const cp::Plan P = cp::plan(rows, any, N);
    CHK(concat_refusal(P.verdict, parts[0]->L));
    CHK(set_dev(parts[0]));
    for (int t = 0; t < n_parts; ++t)   // what was enqueued on a part before the call (a build's tail, a mutation) is in its slabs
        HIPCHK(hipStreamSynchronize(parts[t]->stream));
    lmi_index* c = nullptr;
    if (lmi_create(parts[0]->device, &c) != 0) return fail("lmi_concat: %s", std::string(g_err).c_str());
    if (concat_fill(parts, n_parts, c, P, n_total) != 0) {   // the new handle and everything the call allocated go; the parts were only read
        const std::string why = g_err;
        (void)hipStreamSynchronize(c->stream);
        (void)lmi_destroy(c);
        if (n_total) *n_total = 0;
        for (int64_t& w : g_concat_last) w = 0;
        return fail("lmi_concat: %s; no index was made and the parts are unchanged", why.c_str());
    }
    *out = c;
    return 0;
}
