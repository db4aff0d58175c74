// lmi_host_model.h -- the navigation models on the host side: packing of the Linear stacks, the tree, the MLP forward in its fused
// and per-layer forms (lmi_mlp_topk / lmi_mlp_proba) and the multi-level walk (nav_enqueue, lmi_nav_order).
#pragma once
#include "lmi_host.h"

// upload a row-major host matrix and pack it fragment-major (rows padded to 32, K to 8*KG)
static int pack_from_host(lmi_index* h, const float* src, int rows, int cols, int n_rb, int KG, DevBuf& dst) {
    CHK(h->stage.reserve((size_t)rows * cols * sizeof(float)));
    HIPCHK(hipMemcpyAsync(h->stage.p, src, (size_t)rows * cols * sizeof(float), hipMemcpyHostToDevice, h->stream));
    CHK(dst.reserve((size_t)n_rb * KG * 1024));
    long long total = (long long)n_rb * 32 * KG;
    pack_gather_kernel<<<cdiv(total, 256), 256, 0, h->stream>>>(h->stage.as<float>(), cols, nullptr, rows,
                                                               (long long)n_rb * 32, KG, dst.as<float4>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));  // staging buffer is reused by the next call
    return 0;
}

// packs one Linear stack (torch layout W[out][in]) fragment-major: shared by lmi_set_mlp and lmi_nav_set_model
// (m.n_layers stays 0 -- "no weights" -- until every layer is in place)
static int pack_model(lmi_index* h, const char* who, int n_layers, const int* dims, const float* const* W, const float* const* b, Model& m) {
    h->desc_dirty = true;
    m.n_layers = 0;
    if (n_layers < 1 || n_layers > LMI_MAX_LAYERS) return fail("%s: n_layers %d out of range", who, n_layers);
    for (int i = 0; i <= n_layers; ++i)
        if (dims[i] < 1) return fail("%s: dims[%d] = %d", who, i, dims[i]);
    m.dims.assign(dims, dims + n_layers + 1);
    m.n_rb.assign(n_layers, 0);
    m.KG.assign(n_layers, 0);
    m.Wf.assign(n_layers, DevBuf());   // (the earlier weights go with their buffers)
    m.bias.assign(n_layers, DevBuf());
    for (int i = 0; i < n_layers; ++i) {
        m.n_rb[i] = cdiv(dims[i + 1], 32);
        m.KG[i] = (i == 0) ? cdiv(dims[0], 8) : m.n_rb[i - 1] * 4;  // hidden K = padded features
        if (!W[i] || !b[i]) return fail("%s: NULL weight/bias for layer %d", who, i);
        CHK(pack_from_host(h, W[i], dims[i + 1], dims[i], m.n_rb[i], m.KG[i], m.Wf[i]));
        std::vector<float> bp((size_t)m.n_rb[i] * 32, 0.0f);
        std::copy(b[i], b[i] + dims[i + 1], bp.begin());
        CHK(m.bias[i].reserve(bp.size() * sizeof(float)));
        HIPCHK(hipMemcpy(m.bias[i].p, bp.data(), bp.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    m.n_layers = n_layers;
    return 0;
}

extern "C" LMI_API int lmi_set_mlp(lmi_index* h, int n_layers, const int* dims, const float* const* W,
                           const float* const* b) {
    if (!h) return fail("lmi_set_mlp: NULL handle");
    CHK(set_dev(h));
    return pack_model(h, "lmi_set_mlp", n_layers, dims, W, b, h->models[0]);
}

extern "C" LMI_API int lmi_set_stop_mass(lmi_index* h, float mass) {
    if (!h) return fail("lmi_set_stop_mass: NULL handle");
    if (!(mass >= 0.0f && mass <= 1.0f)) return fail("lmi_set_stop_mass: mass %g outside [0, 1] (0: off)", (double)mass);
    h->stop_mass = mass;
    return 0;
}

extern "C" LMI_API int lmi_set_stop_rows(lmi_index* h, int64_t rows) {
    if (!h) return fail("lmi_set_stop_rows: NULL handle");
    if (rows < 0) return fail("lmi_set_stop_rows: rows %lld is negative (0: off)", (long long)rows);
    h->stop_rows = rows;
    return 0;
}

// What a call that the row-budget stop would cut (rows > 0, n_buckets > 1) needs, checked before anything is launched: the kernels
// read n(b) from d_nb_rows for every class / child bucket they meet, and the counts must be the whole index's.
static int stop_rows_check(lmi_index* h, bool walk, const char* who) {
    if (!h->built)
        return fail("%s: lmi_set_stop_rows is on (%lld) and the handle has no built index: the budget counts the objects of the buckets (lmi_buckets_begin/add_rows/end)",
                    who, (long long)h->stop_rows);
    for (size_t b = 0; b < h->h_owned.size(); ++b)
        if (!h->h_owned[b])
            return fail("%s: lmi_set_stop_rows is on (%lld) and the index was built with an `owned` mask that leaves bucket %zu out: a sharded rank does not know the other ranks' counts",
                        who, (long long)h->stop_rows, b);
    if (!walk) {
        if (h->root().dims.back() > h->L)
            return fail("%s: lmi_set_stop_rows is on (%lld) and the model has %d classes, the index only %d bucket ids", who, (long long)h->stop_rows,
                        h->root().dims.back(), h->L);
    } else {
        for (size_t e = 0; e < h->h_child_bucket.size(); ++e)
            if (h->h_child_bucket[e] >= h->L)
                return fail("%s: lmi_set_stop_rows is on (%lld) and child_bucket[%zu] = %d is no bucket id of the index (%d)", who, (long long)h->stop_rows, e,
                            h->h_child_bucket[e], h->L);
    }
    return 0;
}

// the stops of a 1-level bucket order as the ranking launches take them: mass 0 / rows 0 = that stop is off
struct RankStop {
    float mass = 0.0f;
    long long rows = 0;
    const int* nb_rows = nullptr;   // the index's live counts (rows > 0)
};

// the class ranking behind the per-layer kernels and behind a fused launch whose logits went through global memory: with the row
// budget on rank_classes_rows_kernel (which applies a mass as well), with the mass stop alone rank_classes_stop_kernel takes
// rank_classes_kernel's place
// (LMI_MLP_PLAN_RANK_KERNEL: 0 rank_classes_kernel, 1 rank_classes_stop_kernel, 2 rank_classes_rows_kernel)
static int rank_kernel_of(const RankStop& S) { return S.rows > 0 ? 2 : S.mass > 0.0f ? 1 : 0; }
static int rank_enqueue(lmi_index* h, hipStream_t st, const float* d_logits, int nq, int L, int nb, const RankStop& S, int* d_order) {
    const float mass = S.mass;
    const int kind = rank_kernel_of(S);
    if (kind == 2) rank_classes_rows_kernel<<<nq, 64, 0, st>>>(d_logits, nq, L, nb, mass, S.nb_rows, S.rows, d_order);
    else if (kind == 1) rank_classes_stop_kernel<<<nq, 64, 0, st>>>(d_logits, nq, L, nb, mass, d_order);
    else rank_classes_kernel<<<nq, 64, 0, st>>>(d_logits, nq, L, nb, d_order);
    HIPCHK(hipGetLastError());
    h->last_mlp_plan[LMI_MLP_PLAN_RANK_KERNEL] = kind;
    return 0;
}

extern "C" LMI_API int lmi_set_path_mass(lmi_index* h, float mass) {
    if (!h) return fail("lmi_set_path_mass: NULL handle");
    if (!(mass >= 0.0f && mass <= 1.0f)) return fail("lmi_set_path_mass: mass %g outside [0, 1] (0: off)", (double)mass);
    h->path_mass = mass;
    return 0;
}

extern "C" LMI_API int lmi_set_fused_mlp(lmi_index* h, int on) {
    if (!h) return fail("lmi_set_fused_mlp: NULL handle");
    if (on < 0 || on > 2) return fail("lmi_set_fused_mlp: mode %d outside 0..2", on);
    h->fused_mlp = on;
    return 0;
}

// ---- multi-level index: the internal nodes' models and the tree (lmi_mlp_fused.h) ----
extern "C" LMI_API int lmi_nav_set_model(lmi_index* h, int model_id, int n_layers, const int* dims, const float* const* W,
                                 const float* const* b) {
    if (!h) return fail("lmi_nav_set_model: NULL handle");
    if (model_id < 1 || model_id > 1 << 20) return fail("lmi_nav_set_model: model_id %d (the root, model 0, is lmi_set_mlp)", model_id);
    CHK(set_dev(h));
    if ((size_t)model_id >= h->models.size()) h->models.resize(model_id + 1);
    h->tree_set = false;
    return pack_model(h, "lmi_nav_set_model", n_layers, dims, W, b, h->models[model_id]);
}

// every model of a tree reads the same query rows: the walk hands mlp_fused_kernel ONE input width (the root's, fused_base) while a
// node's layer 0 is packed for its own dims[0], so a node of another width would be evaluated on the wrong features without a fault.
// Checked when the tree is set and again before every walk (lmi_set_mlp may replace the root under a tree that was set).
static int tree_widths_check(const lmi_index* h, const char* who) {
    const int d = h->root().dims[0];
    for (size_t m = 1; m < h->models.size(); ++m)
        if (h->models[m].n_layers > 0 && h->models[m].dims[0] != d)
            return fail("%s: model %zu takes %d input features, the root model %d: every model of a tree reads the same queries", who, m,
                        h->models[m].dims[0], d);
    return 0;
}

extern "C" LMI_API int lmi_nav_set_tree(lmi_index* h, int n_models, const int32_t* child_offset, const int32_t* child_model,
                                const int32_t* child_bucket) {
    if (!h) return fail("lmi_nav_set_tree: NULL handle");
    if (h->root().n_layers == 0) return fail("lmi_nav_set_tree: no root model (lmi_set_mlp)");
    if (n_models != (int)h->models.size()) return fail("lmi_nav_set_tree: %d models, %d set (root + lmi_nav_set_model)", n_models, (int)h->models.size());
    CHK(tree_widths_check(h, "lmi_nav_set_tree"));
    if (!child_offset || !child_model || !child_bucket || child_offset[0] != 0) return fail("lmi_nav_set_tree: bad arguments");
    for (int m = 0; m < n_models; ++m) {
        if (h->models[m].n_layers == 0) return fail("lmi_nav_set_tree: model %d has no weights (lmi_nav_set_model)", m);
        const int classes = h->models[m].dims.back();
        if (child_offset[m + 1] - child_offset[m] != classes) return fail("lmi_nav_set_tree: model %d has %d classes, %d children listed", m, classes, child_offset[m + 1] - child_offset[m]);
    }
    const int total = child_offset[n_models];
    for (int e = 0; e < total; ++e) {
        if (child_model[e] < -1 || child_model[e] == 0 || child_model[e] >= n_models) return fail("lmi_nav_set_tree: child_model[%d] = %d", e, child_model[e]);
        if (child_bucket[e] < -2) return fail("lmi_nav_set_tree: child_bucket[%d] = %d", e, child_bucket[e]);
    }
    CHK(set_dev(h));
    h->h_child_offset.assign(child_offset, child_offset + n_models + 1);
    h->h_child_model.assign(child_model, child_model + total);
    h->h_child_bucket.assign(child_bucket, child_bucket + total);
    CHK(h->d_child_offset.reserve((size_t)(n_models + 1) * 4));
    CHK(h->d_child_model.reserve((size_t)std::max(total, 1) * 4));
    CHK(h->d_child_bucket.reserve((size_t)std::max(total, 1) * 4));
    HIPCHK(hipMemcpy(h->d_child_offset.p, child_offset, (size_t)(n_models + 1) * 4, hipMemcpyHostToDevice));
    if (total) {
        HIPCHK(hipMemcpy(h->d_child_model.p, child_model, (size_t)total * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(h->d_child_bucket.p, child_bucket, (size_t)total * 4, hipMemcpyHostToDevice));
    }
    h->tree_set = true;
    return 0;
}

// the LDS plan of mlp_fused_kernel for a model set, from the models' shapes alone (build_descs and lmi_debug_mlp_plan)
struct FusedLds {
    bool ok = true;           // every model fits the fused kernel
    bool logits_lds = true;   // every model's last layer keeps its outputs in LDS
    int s0 = 1, s1 = 1;       // strides of the two activation buffers: the widest padded layer of either parity, + 1
    int lds = 0;              // bytes
};
static FusedLds fused_lds_plan(const std::vector<Model>& models) {
    FusedLds F;
    int w0 = 0, w1 = 0;
    for (const Model& M : models) {
        if (M.n_layers == 0) { F.ok = false; continue; }
        for (int i = 0; i < M.n_layers; ++i) {
            const int padded = M.n_rb[i] * 32;
            const bool last = i + 1 == M.n_layers;
            if (padded > FM_MAXH) { if (last) F.logits_lds = false; else F.ok = false; continue; }
            int& wref = (i & 1) ? w1 : w0;
            wref = std::max(wref, padded);
        }
    }
    F.s0 = w0 + 1;
    F.s1 = w1 + 1;
    F.lds = (2 * FM_COLS * FM_CHUNK_S + FM_COLS * F.s0 + FM_COLS * F.s1) * 4;
    // (cannot fire while the widths kept in LDS are capped at FM_MAXH = 512: 24 832 + 128 (w0 + w1 + 2) <= 156 160 < 162 816)
    if (F.lds > 160 * 1024 - 1024) F.ok = false;
    return F;
}

// device descriptors of every model + the LDS plan of mlp_fused_kernel for the current model set
static int build_descs(lmi_index* h) {
    if (!h->desc_dirty) return 0;
    const int nm = (int)h->models.size();
    std::vector<ModelDesc> D(nm);
    for (int m = 0; m < nm; ++m) {
        const Model& M = h->models[m];
        ModelDesc& d = D[m];
        memset(&d, 0, sizeof(d));
        d.n_layers = M.n_layers;
        if (M.n_layers == 0) continue;
        for (int i = 0; i <= M.n_layers; ++i) d.dims[i] = M.dims[i];
        for (int i = 0; i < M.n_layers; ++i) {
            d.KG[i] = M.KG[i];
            d.W[i] = M.Wf[i].as<float4>();
            d.b[i] = M.bias[i].as<float>();
        }
    }
    const FusedLds F = fused_lds_plan(h->models);
    const bool ok = F.ok;
    h->fm_s0 = F.s0;
    h->fm_s1 = F.s1;
    h->fm_act0 = FM_COLS * h->fm_s0;
    h->fm_lds = F.lds;
    h->fm_ok = ok;
    h->fm_logits_lds = F.logits_lds ? 1 : 0;
    CHK(h->d_models.reserve(sizeof(ModelDesc) * nm));
    HIPCHK(hipMemcpy(h->d_models.p, D.data(), sizeof(ModelDesc) * nm, hipMemcpyHostToDevice));
    if (ok) {
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&mlp_fused_kernel<FM_TOPK>), hipFuncAttributeMaxDynamicSharedMemorySize, h->fm_lds));
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&mlp_fused_kernel<FM_PROBA>), hipFuncAttributeMaxDynamicSharedMemorySize, h->fm_lds));
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&mlp_fused_kernel<FM_NAV>), hipFuncAttributeMaxDynamicSharedMemorySize, h->fm_lds));
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&mlp_fused_kernel<FM_TOPK_STOP>), hipFuncAttributeMaxDynamicSharedMemorySize, h->fm_lds));
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&mlp_fused_kernel<FM_NAV_MASS>), hipFuncAttributeMaxDynamicSharedMemorySize, h->fm_lds));
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&mlp_fused_kernel<FM_TOPK_ROWS>), hipFuncAttributeMaxDynamicSharedMemorySize, h->fm_lds));
    }
    h->desc_dirty = false;
    return 0;
}

static void fused_base(lmi_index* h, const float* d_q, int nq, FusedParams& P) {
    memset(&P, 0, sizeof(P));
    P.models = h->d_models.as<ModelDesc>();
    P.n_models = (int)h->models.size();
    P.x = d_q;
    P.d = h->root().dims[0];
    P.nq = nq;
    P.s0 = h->fm_s0;
    P.s1 = h->fm_s1;
    P.act0_floats = h->fm_act0;
    P.logits_in_lds = h->fm_logits_lds;
}

// ---- the MLP forward's dispatch.  mlp_plan() decides which form a batch takes; the functions below it are the instances the
// launch sites pick on top.  Each is ONE function, called by the launch and by the plan report (mlp_plan_report,
// lmi_debug_mlp_plan), so that the report cannot drift from the launch ----
struct MlpPlan {
    int fused = 0;            // a mlp_fused_kernel launch
    int mode = -1;            // its FM_* instance
    int grid = 0;             // its blocks
    int nq_head = 0;          // the queries it takes
    int layers_queries = 0;   // the queries of the mlp_layer_kernel chain (a split batch's tail, or the whole batch)
};
// fm_ok / logits_lds: the model set's LDS plan (fused_lds_plan); proba: lmi_mlp_proba; want_logits: the caller takes the logits
static MlpPlan mlp_plan(int num_cus, int fused_mlp, bool fm_ok, bool logits_lds, int nq, bool proba, bool want_logits, const RankStop& stop) {
    MlpPlan P;
    // One launch for every layer + ranking when the batch fills the chip (a block = 32 queries, one per CU for the wide
    // models: 8 192 queries 100 us against 138 us for the per-layer kernels); small batches (a rank's slice of a
    // sharded batch, single queries) have too few 32-query blocks for that and take the per-layer kernels, whose grids
    // also split the features (2 048 queries: 79 us against 88 us).  predict_proba always takes the fused kernel.
    const bool fill = cdiv(nq, FM_COLS) * 2 >= num_cus || proba || fused_mlp == 2;
    if (!(fused_mlp && fm_ok && fill)) {
        P.layers_queries = nq;
        return P;
    }
    // every layer, the ranking and the softmax in ONE launch (lmi_mlp_fused.h)
    // A batch whose last round of 32-query blocks would fill under 30 % of the CUs (10 000 queries: 313 blocks = 256 + 57)
    // pays a whole second round for it.  The tail's queries go through the per-layer kernels on a side stream instead,
    // beside the fused kernel's one full round (the fused blocks leave wave slots and half of the MFMA pipe): 182 ->
    // ~125 us at 10 000 queries; identical results (both forms are the canonical chain).
    P.fused = 1;
    P.mode = proba ? FM_PROBA : stop.rows > 0 ? FM_TOPK_ROWS : stop.mass > 0.0f ? FM_TOPK_STOP : FM_TOPK;
    P.grid = cdiv(nq, FM_COLS);
    P.nq_head = nq;
    const int rem = P.grid % num_cus;
    if (fused_mlp == 1 && !proba && !want_logits && logits_lds && P.grid > num_cus && rem > 0 && rem * 10 < num_cus * 3) {
        P.nq_head = (P.grid - rem) * FM_COLS;
        P.grid -= rem;
        P.layers_queries = nq - P.nq_head;
    }
    return P;
}
// mlp_layer_kernel<LAST, CBW>: col-blocks per wave: 4 when that already gives every CU two blocks, else 2, else 1 (e.g. the
// 120-class output layer has 4 feature blocks = one block row; 768->512 on 10 000 queries had 316 blocks of CBW 4 on 256 CUs)
static int mlp_layer_cbw(int num_cus, int n_rb, int ncb) {
    const int rows = cdiv(n_rb, 4);
    return rows * cdiv(ncb, 4) >= 2 * num_cus ? 4 : rows * cdiv(ncb, 2) >= 2 * num_cus ? 2 : 1;
}
// mlp_fused_kernel's layer 0, restated for the report: whole chunks are fetched as float4 when the rows are 16-byte multiples,
// and the input goes through LDS in chunks of FM_CHUNK features
static int fused_vec_in(int d) { return (d & 3) == 0; }
static int fused_in_chunks(int KG0) { return cdiv(KG0 * 8, FM_CHUNK); }

// MLP forward + class ranking (+ softmax when d_probs: then nb == L and d_order receives the full class order)
// the per-layer form: one mlp_layer_kernel launch per Linear, then the ranking (and softmax) kernels, on stream `st`
// stop: the order is cut by the probability-mass stop and / or the row budget (never together with d_probs)
static int mlp_layers_enqueue(lmi_index* h, hipStream_t st, const float* d_q, int nq, int nb, int* d_order, float* d_logits_out, float* d_probs,
                              const RankStop& stop) {
    const Model& R = h->root();
    const int L = R.dims[R.n_layers];
    const int ncb = cdiv(nq, 32);
    // pack the queries as the B operand of layer 0
    CHK(h->xfrag.reserve((size_t)ncb * R.KG[0] * 1024));
    {
        long long total = (long long)ncb * 32 * R.KG[0];
        pack_gather_kernel<<<cdiv(total, 256), 256, 0, st>>>(d_q, R.dims[0], nullptr, nq, (long long)ncb * 32,
                                                            R.KG[0], h->xfrag.as<float4>(), st == h->stream ? tsp(h, ST_MLP0) : nullptr);
        HIPCHK(hipGetLastError());
    }
    int maxrb = 0;
    for (int i = 0; i + 1 < R.n_layers; ++i) maxrb = std::max(maxrb, R.n_rb[i]);
    for (int i = 0; i < 2; ++i) CHK(h->act[i].reserve((size_t)std::max(1, ncb) * std::max(1, maxrb) * 4 * 1024));
    float* d_logits = d_logits_out;
    if (!d_logits) {
        CHK(h->logits.reserve((size_t)nq * L * 4));
        d_logits = h->logits.as<float>();
    }
    const float4* in = h->xfrag.as<float4>();
    for (int i = 0; i < R.n_layers; ++i) {
        const bool last = i + 1 == R.n_layers;
        const int rows = cdiv(R.n_rb[i], 4);
        const int cbw = mlp_layer_cbw(h->num_cus, R.n_rb[i], ncb);
        h->last_mlp_plan[LMI_MLP_PLAN_CBW0 + i] = cbw;
        dim3 grid(cdiv(ncb, cbw), rows);
        float* o = last ? d_logits : h->act[i & 1].as<float>();
        const int KGn = last ? 0 : R.n_rb[i] * 4;
#define LMI_MLP_LAUNCH(LASTV, CBWV)                                                                        \
        mlp_layer_kernel<LASTV, CBWV><<<grid, 256, 0, st>>>(R.Wf[i].as<float4>(), R.bias[i].as<float>(), in, \
                                                           R.KG[i], R.n_rb[i], ncb, o, KGn, nq, L)
        if (last) {
            if (cbw == 4) LMI_MLP_LAUNCH(true, 4); else if (cbw == 2) LMI_MLP_LAUNCH(true, 2); else LMI_MLP_LAUNCH(true, 1);
        } else {
            if (cbw == 4) LMI_MLP_LAUNCH(false, 4); else if (cbw == 2) LMI_MLP_LAUNCH(false, 2); else LMI_MLP_LAUNCH(false, 1);
            in = reinterpret_cast<const float4*>(o);
        }
#undef LMI_MLP_LAUNCH
        HIPCHK(hipGetLastError());
    }
    CHK(rank_enqueue(h, st, d_logits, nq, L, nb, stop, d_order));
    if (d_probs) {
        softmax_ranked_kernel<<<cdiv(nq, 64), 64, 0, st>>>(d_logits, d_order, nq, L, d_probs);
        HIPCHK(hipGetLastError());
        h->last_mlp_plan[LMI_MLP_PLAN_SOFTMAX_KERNEL] = 1;
    }
    return 0;
}

// what mlp_enqueue and lmi_debug_mlp_plan check alike, behind the caller's name, and the stops a bucket order of nb ranks is cut by
static int mlp_call_check(lmi_index* h, int nb, bool proba, const char* who, RankStop& stop) {
    if (h->root().n_layers == 0) return fail("%s: no MLP set (lmi_set_mlp)", who);
    const int L = h->root().dims.back();
    if (nb < 1 || nb > L) return fail("%s: n_buckets %d outside [1,%d]", who, nb, L);
    // the probability-mass stop (lmi_set_stop_mass) cuts a bucket order; predict_proba's full class order and a single rank are never cut
    stop.mass = (!proba && nb > 1) ? h->stop_mass : 0.0f;
    // the row budget (lmi_set_stop_rows) likewise; both halves of a split batch and every ranking path take the same `stop`
    stop.rows = (!proba && nb > 1) ? (long long)h->stop_rows : 0;
    if (stop.rows > 0) {
        CHK(stop_rows_check(h, false, who));
        stop.nb_rows = h->d_nb_rows.as<int>();
    }
    return 0;
}

// The LMI_MLP_PLAN_* words of a forward (include/lmi_hip.h).  mlp_plan_record: the plan's fields, as mlp_enqueue starts the handle's
// record (every launch site then writes its own words as it launches); mlp_plan_report: the sites' words as well, from the same
// functions the sites call, for the sites this plan reaches -- what lmi_debug_mlp_plan returns.
static_assert(LMI_MLP_PLAN_COUNT <= CallState::PLAN_WORDS, "lmi_handle.h holds the plan words");
static_assert(LMI_MLP_PLAN_CBW7 - LMI_MLP_PLAN_CBW0 + 1 == LMI_MAX_LAYERS, "one CBW word per layer");
static void mlp_plan_record(const lmi_index* h, const FusedLds& F, const MlpPlan& P, int32_t* w) {
    for (int i = 0; i < LMI_MLP_PLAN_COUNT; ++i) w[i] = -1;
    w[LMI_MLP_PLAN_NUM_CUS] = h->num_cus; w[LMI_MLP_PLAN_FM_OK] = F.ok; w[LMI_MLP_PLAN_LOGITS_LDS] = F.logits_lds;
    w[LMI_MLP_PLAN_LDS_BYTES] = F.lds; w[LMI_MLP_PLAN_FUSED] = P.fused; w[LMI_MLP_PLAN_MODE] = P.mode;
    w[LMI_MLP_PLAN_FUSED_BLOCKS] = P.grid; w[LMI_MLP_PLAN_NQ_HEAD] = P.nq_head; w[LMI_MLP_PLAN_LAYERS_QUERIES] = P.layers_queries;
    w[LMI_MLP_PLAN_SOFTMAX_KERNEL] = 0;
}
static void mlp_plan_report(const lmi_index* h, const FusedLds& F, const MlpPlan& P, const RankStop& stop, bool proba, int32_t* w) {
    mlp_plan_record(h, F, P, w);
    const Model& R = h->root();
    if (P.fused) {
        w[LMI_MLP_PLAN_VEC_IN] = fused_vec_in(R.dims[0]);
        w[LMI_MLP_PLAN_IN_CHUNKS] = fused_in_chunks(R.KG[0]);
    }
    if (P.layers_queries > 0)
        for (int i = 0; i < R.n_layers; ++i) w[LMI_MLP_PLAN_CBW0 + i] = mlp_layer_cbw(h->num_cus, R.n_rb[i], cdiv(P.layers_queries, 32));
    if (P.layers_queries > 0 || !F.logits_lds) {
        w[LMI_MLP_PLAN_RANK_KERNEL] = rank_kernel_of(stop);
        w[LMI_MLP_PLAN_SOFTMAX_KERNEL] = proba;
    }
}

static int mlp_enqueue(lmi_index* h, const float* d_q, int nq, int nb, int* d_order, float* d_logits_out, float* d_probs = nullptr) {
    RankStop stop;
    CHK(mlp_call_check(h, nb, d_probs != nullptr, "lmi_mlp_topk", stop));
    const int L = h->root().dims.back();
    CHK(build_descs(h));
    const float mass = stop.mass;
    const MlpPlan plan = mlp_plan(h->num_cus, h->fused_mlp, h->fm_ok, h->fm_logits_lds != 0, nq, d_probs != nullptr, d_logits_out != nullptr, stop);
    {
        FusedLds F;   // (build_descs keeps fused_lds_plan's answer in the handle)
        F.ok = h->fm_ok; F.logits_lds = h->fm_logits_lds != 0; F.s0 = h->fm_s0; F.s1 = h->fm_s1; F.lds = h->fm_lds;
        mlp_plan_record(h, F, plan, h->last_mlp_plan);   // (the launch sites add their words)
    }
    if (plan.fused) {
        const int grid = plan.grid, nq_head = plan.nq_head;
        FusedParams P;
        fused_base(h, d_q, nq_head, P);
        float* d_logits = d_logits_out;
        if (!h->fm_logits_lds && !d_logits) {  // wide output layer: logits through global memory, ranked below
            CHK(h->logits.reserve((size_t)nq * L * 4));
            d_logits = h->logits.as<float>();
        }
        P.logits_out = d_logits;
        P.nb = nb;
        P.order = d_order;
        P.probs = d_probs;
        P.classes = d_order;
        P.ts = tsp(h, ST_MLP0);
        P.stop_mass = mass;
        P.nb_rows = stop.nb_rows;
        P.stop_rows = stop.rows;
        if (nq_head < nq) CHK(side_fork(h));
        if (plan.mode == FM_PROBA) mlp_fused_kernel<FM_PROBA><<<grid, 256, h->fm_lds, h->stream>>>(P);
        else if (plan.mode == FM_TOPK_ROWS) mlp_fused_kernel<FM_TOPK_ROWS><<<grid, 256, h->fm_lds, h->stream>>>(P);
        else if (plan.mode == FM_TOPK_STOP) mlp_fused_kernel<FM_TOPK_STOP><<<grid, 256, h->fm_lds, h->stream>>>(P);
        else mlp_fused_kernel<FM_TOPK><<<grid, 256, h->fm_lds, h->stream>>>(P);
        HIPCHK(hipGetLastError());
        h->last_mlp_plan[LMI_MLP_PLAN_VEC_IN] = fused_vec_in(P.d);
        h->last_mlp_plan[LMI_MLP_PLAN_IN_CHUNKS] = fused_in_chunks(h->root().KG[0]);
        if (nq_head < nq) {
            CHK(mlp_layers_enqueue(h, h->side, d_q + (size_t)nq_head * h->root().dims[0], nq - nq_head, nb, d_order + (size_t)nq_head * nb, nullptr, nullptr, stop));
            CHK(side_join(h));
        }
        if (!h->fm_logits_lds) {
            CHK(rank_enqueue(h, h->stream, d_logits, nq, L, nb, stop, d_order));
            if (d_probs) {
                softmax_ranked_kernel<<<cdiv(nq, 64), 64, 0, h->stream>>>(d_logits, d_order, nq, L, d_probs);
                HIPCHK(hipGetLastError());
                h->last_mlp_plan[LMI_MLP_PLAN_SOFTMAX_KERNEL] = 1;
            }
        }
        return 0;
    }
    return mlp_layers_enqueue(h, h->stream, d_q, nq, nb, d_order, d_logits_out, d_probs, stop);
}

// lmi_mlp_topk and (q16) lmi_mlp_topk_f16: the halves take lmi_search_f16's front -- uploaded as they are, widened on the device into
// q_nav (input_ptr16) -- and from there on the call is the binary32 call on the widened values
static int mlp_topk_impl(lmi_index* h, const void* queries_nav, int q16, int nq, int nb, int32_t* bucket_order, float* logits, int on_device) {
    const char* who = q16 ? "lmi_mlp_topk_f16" : "lmi_mlp_topk";
    if (!h) return fail("%s: NULL handle", who);
    if (nq < 0) return fail("%s: nq < 0", who);
    if (nq == 0) return 0;
    CHK(set_dev(h));
    if (h->root().n_layers == 0) return fail("%s: no MLP set (lmi_set_mlp)", who);
    const int L = h->root().dims.back();
    const void* d_q = nullptr;
    if (q16) CHK(input_ptr16(h, queries_nav, nq, h->root().dims[0], on_device, h->q16_nav, h->q_nav, &d_q));
    else CHK(input_ptr(h, queries_nav, (size_t)nq * h->root().dims[0] * 4, on_device, h->q_nav, &d_q));
    int* d_order = bucket_order;
    float* d_logits = logits;
    if (!on_device) {
        CHK(h->order.reserve((size_t)nq * nb * 4));
        d_order = h->order.as<int>();
        if (logits) { CHK(h->logits.reserve((size_t)nq * L * 4)); d_logits = h->logits.as<float>(); }
    }
    begin_call(h);
    CHK(record(h, 0));
    CHK(mlp_enqueue(h, static_cast<const float*>(d_q), nq, nb, d_order, d_logits));
    CHK(record(h, 1));
    CHK(stamp_end(h, ST_MLP1));
    if (!on_device) CHK(copy_back(h, {{bucket_order, d_order, (size_t)nq * nb * 4}, {logits, d_logits, (size_t)nq * L * 4}}));
    return 0;
}

extern "C" LMI_API int lmi_mlp_topk(lmi_index* h, const float* queries_nav, int nq, int nb, int32_t* bucket_order,
                            float* logits, int on_device) {
    return mlp_topk_impl(h, queries_nav, 0, nq, nb, bucket_order, logits, on_device);
}
extern "C" LMI_API int lmi_mlp_topk_f16(lmi_index* h, const uint16_t* queries_nav, int nq, int nb, int32_t* bucket_order,
                                float* logits, int on_device) {
    return mlp_topk_impl(h, queries_nav, 1, nq, nb, bucket_order, logits, on_device);
}

extern "C" LMI_API int lmi_mlp_proba(lmi_index* h, const float* queries_nav, int nq, float* probs, int32_t* classes,
                             int on_device) {
    if (!h) return fail("lmi_mlp_proba: NULL handle");
    if (nq < 0) return fail("lmi_mlp_proba: nq < 0");
    if (nq == 0) return 0;
    CHK(set_dev(h));
    if (h->root().n_layers == 0) return fail("lmi_mlp_proba: no MLP set (lmi_set_mlp)");
    const int L = h->root().dims.back();
    const void* d_q = nullptr;
    CHK(input_ptr(h, queries_nav, (size_t)nq * h->root().dims[0] * 4, on_device, h->q_nav, &d_q));
    int* d_order = classes;
    float* d_probs = probs;
    if (!on_device) {
        CHK(h->order.reserve((size_t)nq * L * 4));
        CHK(h->out_d.reserve((size_t)nq * L * 4));
        d_order = h->order.as<int>();
        d_probs = h->out_d.as<float>();
    }
    begin_call(h);
    CHK(record(h, 0));
    CHK(mlp_enqueue(h, static_cast<const float*>(d_q), nq, L, d_order, nullptr, d_probs));
    CHK(record(h, 1));
    CHK(stamp_end(h, ST_MLP1));
    if (!on_device) CHK(copy_back(h, {{classes, d_order, (size_t)nq * L * 4}, {probs, d_probs, (size_t)nq * L * 4}}));
    return 0;
}

// Multi-level navigation on the device: LearnedIndex._precompute_bucket_order for len(n_categories) > 1
// (LearnedIndex.py:216-252) -- the batched priority-queue walk.  slab_ids[nq][nb] <- slab bucket id of the
// j-th visited bucket (-1: listed bucket without objects or queue exhausted), entries[nq][nb] <- its flat child
// index (child_offset[parent model] + class; -1: none) from which the caller rebuilds the path.
// The multi-level walk of one batch, enqueued on h->stream: d_slab / d_ent [nq][nb] receive the visited buckets in visiting order.
// Trees of up to NAV_ENQUEUE_ALL models: EVERY possible step is enqueued up front and a step whose predecessor left no query waiting
// returns at once (nav_pop_kernel: prev_active) -- no host round trip inside the walk, the call is asynchronous like every other
// enqueue.  Larger trees: steps in batches of 4 with the count read back after each (one small synchronisation).
// The path-mass stop (lmi_set_path_mass > 0): the same launches in their mass forms (mlp_fused_kernel<FM_NAV_MASS>, nav_pop_mass_kernel /
// nav_pop_lds_mass_kernel) with three more buffers; a single bucket per query (nb == 1) is never cut, so it takes the plain forms.
// The row-budget stop (lmi_set_stop_rows > 0): the pop kernels in their rows forms (nav_pop_rows_kernel / nav_pop_lds_rows_kernel; with
// a path mass as well nav_pop_mass_rows_kernel / nav_pop_lds_mass_rows_kernel) with one more buffer; the MLP launches are untouched.
constexpr int NAV_ENQUEUE_ALL = 16;
static int nav_check(lmi_index* h, int nq, int nb, const char* who) {
    if (!h->tree_set) return fail("%s: no tree (lmi_nav_set_model / lmi_nav_set_tree)", who);
    if (h->root().n_layers == 0) return fail("%s: no root model (lmi_set_mlp)", who);
    CHK(tree_widths_check(h, who));
    CHK(set_dev(h));
    CHK(build_descs(h));
    if (!h->fm_ok || !h->fm_logits_lds)
        return fail("%s: a model of the tree does not fit the fused kernel (layer outputs <= %d, LDS plan %d bytes)", who, FM_MAXH, h->fm_lds);
    const int nm = (int)h->models.size();
    const int cap = h->h_child_offset[nm];
    if ((long long)nq * cap >= (1ll << 31) || (long long)nq * nb >= (1ll << 31)) return fail("%s: nq too large for this tree", who);
    if (cap == 0) return fail("%s: empty tree", who);
    return 0;
}
static int nav_enqueue(lmi_index* h, const float* d_q, int nq, int nb, int* d_slab, int* d_ent) {
    const int nm = (int)h->models.size();
    const int cap = h->h_child_offset[nm];
    const bool with_rows = h->stop_rows > 0 && nb > 1;
    if (with_rows) CHK(stop_rows_check(h, true, "lmi_nav_order"));
    CHK(h->pq_prob.reserve((size_t)nq * cap * 4));
    CHK(h->pq_ent.reserve((size_t)nq * cap * 4));
    CHK(h->pq_len.reserve((size_t)nq * 4));
    CHK(h->nav_len.reserve((size_t)nq * 4));
    CHK(h->nav_count.reserve((size_t)2 * (nm + 1) * 4));  // [2][nm + 1]: per-model counters + the step's active-query count
    CHK(h->nav_colq.reserve((size_t)nm * nq * 4));
    const bool with_mass = h->path_mass > 0.0f && nb > 1;
    if (with_mass) {
        CHK(h->pq_mass.reserve((size_t)nq * cap * 4));
        CHK(h->nav_parent_mass.reserve((size_t)nq * 4));
        CHK(h->nav_cum.reserve((size_t)nq * 4));
    }
    if (with_rows) CHK(h->nav_rows.reserve((size_t)nq * 8));
    FillRanges Z;
    Z.count = 0;
    bool fill_ok = true;
    auto fill = [&](void* ptr, long long words, unsigned value) { fill_ok = Z.add(ptr, words, value) && fill_ok; };
    fill(h->pq_len.p, nq, 0u);
    fill(h->nav_len.p, nq, 0u);
    fill(d_slab, (long long)nq * nb, 0xFFFFFFFFu);
    fill(d_ent, (long long)nq * nb, 0xFFFFFFFFu);
    fill(h->nav_count.p, 2 * (nm + 1), 0u);
    if (with_mass) {
        fill(h->nav_cum.p, nq, 0u);
        fill(h->nav_parent_mass.p, nq, 0x3F800000u);  // 1.0f: the root's children get their own probability as their mass
    }
    if (with_rows) fill(h->nav_rows.p, 2ll * nq, 0u);   // int64 sums: two words each (8 ranges at the most, FillRanges::MAXR is 12)
    if (!fill_ok) return fail("internal: more than %d fill ranges queued (%s:%d)", FillRanges::MAXR, __FILE__, __LINE__);
    Z.ts = tsp(h, ST_MLP0);
    fill_ranges_kernel<<<h->num_cus * 2, 256, 0, h->stream>>>(Z);
    HIPCHK(hipGetLastError());
    FusedParams P;
    fused_base(h, d_q, nq, P);
    P.pq_prob = h->pq_prob.as<float>();
    P.pq_ent = h->pq_ent.as<int>();
    P.pq_len = h->pq_len.as<int>();
    P.cap = cap;
    P.child_offset = h->d_child_offset.as<int>();
    P.reverse = 1;  // root children: least probable first (LearnedIndex.py:220-227)
    if (with_mass) {
        P.pq_mass = h->pq_mass.as<float>();
        P.parent_mass = h->nav_parent_mass.as<float>();
        mlp_fused_kernel<FM_NAV_MASS><<<cdiv(nq, FM_COLS), 256, h->fm_lds, h->stream>>>(P);
    } else {
        mlp_fused_kernel<FM_NAV><<<cdiv(nq, FM_COLS), 256, h->fm_lds, h->stream>>>(P);
    }
    HIPCHK(hipGetLastError());
    P.reverse = 0;
    P.col_query = h->nav_colq.as<int>();
    NavParams N;
    N.nq = nq; N.nb = nb; N.cap = cap;
    N.pq_prob = P.pq_prob; N.pq_ent = P.pq_ent; N.pq_len = P.pq_len;
    N.child_model = h->d_child_model.as<int>();
    N.child_bucket = h->d_child_bucket.as<int>();
    N.out_len = h->nav_len.as<int>();
    N.out_slab = d_slab;
    N.out_ent = d_ent;
    N.col_query = h->nav_colq.as<int>();
    NavMass S;
    memset(&S, 0, sizeof(S));
    if (with_mass) {
        S.pq_mass = h->pq_mass.as<float>();
        S.cum = h->nav_cum.as<float>();
        S.parent_mass = h->nav_parent_mass.as<float>();
        S.mass = h->path_mass;
    }
    NavRows W;
    memset(&W, 0, sizeof(W));
    if (with_rows) {
        W.nb_rows = h->d_nb_rows.as<int>();
        W.acc = h->nav_rows.as<long long>();
        W.rows = h->stop_rows;
    }
    int* counts = h->nav_count.as<int>();
    // A step pops entries until the query hits an internal node; a query expands each node at most once, so there are
    // at most (models) steps.
    const int max_steps = nm + 1;
    const bool all = nm <= NAV_ENQUEUE_ALL;
    const bool pop_lds = cap <= NAV_LDS_CAP;
    int h_active = 1;
    for (int it = 0; it < max_steps && h_active > 0;) {
        int last_par = 0;
        for (int k4 = 0; (all || k4 < 4) && it < max_steps; ++k4, ++it) {
            const int par = it & 1;
            N.node_count = counts + par * (nm + 1);
            N.active = counts + par * (nm + 1) + nm;
            N.prev_active = (all && it > 0) ? counts + (1 - par) * (nm + 1) + nm : nullptr;
            if (with_mass && with_rows) {
                if (pop_lds) nav_pop_lds_mass_rows_kernel<<<cdiv(nq, 64), 64, (size_t)cap * 64 * 8, h->stream>>>(N, S, W);
                else nav_pop_mass_rows_kernel<<<cdiv(nq, 256), 256, 0, h->stream>>>(N, S, W);
            } else if (with_rows) {
                if (pop_lds) nav_pop_lds_rows_kernel<<<cdiv(nq, 64), 64, (size_t)cap * 64 * 8, h->stream>>>(N, W);
                else nav_pop_rows_kernel<<<cdiv(nq, 256), 256, 0, h->stream>>>(N, W);
            } else if (with_mass) {
                if (pop_lds) nav_pop_lds_mass_kernel<<<cdiv(nq, 64), 64, (size_t)cap * 64 * 8, h->stream>>>(N, S);
                else nav_pop_mass_kernel<<<cdiv(nq, 256), 256, 0, h->stream>>>(N, S);
            } else {
                if (pop_lds) nav_pop_lds_kernel<<<cdiv(nq, 64), 64, (size_t)cap * 64 * 8, h->stream>>>(N);
                else nav_pop_kernel<<<cdiv(nq, 256), 256, 0, h->stream>>>(N);
            }
            HIPCHK(hipGetLastError());
            P.node_count = N.node_count;
            P.zero_counts = counts + (1 - par) * (nm + 1);
            P.n_zero = nm + 1;
            if (with_mass) mlp_fused_kernel<FM_NAV_MASS><<<cdiv(nq, FM_COLS) + nm, 256, h->fm_lds, h->stream>>>(P);
            else mlp_fused_kernel<FM_NAV><<<cdiv(nq, FM_COLS) + nm, 256, h->fm_lds, h->stream>>>(P);
            HIPCHK(hipGetLastError());
            last_par = par;
        }
        if (all) break;
        HIPCHK(hipMemcpyAsync(&h_active, counts + last_par * (nm + 1) + nm, 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    return 0;
}

extern "C" LMI_API int lmi_nav_order(lmi_index* h, const float* queries_nav, int nq, int nb, int32_t* slab_ids, int32_t* entries,
                             int on_device) {
    if (!h) return fail("lmi_nav_order: NULL handle");
    if (nq < 0 || nb < 1) return fail("lmi_nav_order: bad nq/n_buckets");
    if (nq == 0) return 0;
    CHK(nav_check(h, nq, nb, "lmi_nav_order"));
    const void* d_q = nullptr;
    CHK(input_ptr(h, queries_nav, (size_t)nq * h->root().dims[0] * 4, on_device, h->q_nav, &d_q));
    CHK(h->nav_slab.reserve((size_t)nq * nb * 4));
    CHK(h->nav_ent.reserve((size_t)nq * nb * 4));
    int* d_slab = on_device ? slab_ids : h->nav_slab.as<int>();
    int* d_ent = on_device ? entries : h->nav_ent.as<int>();
    begin_call(h);
    CHK(record(h, 0));
    CHK(nav_enqueue(h, static_cast<const float*>(d_q), nq, nb, d_slab, d_ent));
    CHK(record(h, 1));
    CHK(stamp_end(h, ST_MLP1));
    if (!on_device) CHK(copy_back(h, {{slab_ids, d_slab, (size_t)nq * nb * 4}, {entries, d_ent, (size_t)nq * nb * 4}}));
    return 0;
}
