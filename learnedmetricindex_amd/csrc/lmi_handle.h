// lmi_handle.h -- error reporting, the growing device buffer and the handle (lmi_index), which is composed of one part per kind of
// state.  The parts say who owns what: a clone view copies the first five and starts with a call state of its own (clone_handle).
// Host only: the HIP runtime's API and the standard library, no kernel header.
#pragma once
#include <hip/hip_runtime_api.h>

#include <atomic>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

namespace {

thread_local std::string g_err;

int fail(const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return -1;
}

#define HIPCHK(expr)                                                                                \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess)                                                                       \
            return fail("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

#define CHK(expr)              \
    do {                       \
        int r_ = (expr);       \
        if (r_ != 0) return r_; \
    } while (0)

}  // namespace

// device buffer that only grows.  It frees what it owns when it goes; its COPY is a borrowed view of the same memory (a clone view's
// models and index images: never freed, never grown); a move hands the memory on and leaves the source empty.
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    bool borrowed = false;  // the memory belongs to the buffer this one was copied from
    DevBuf() = default;
    DevBuf(const DevBuf& o) : p(o.p), cap(o.cap), borrowed(o.p != nullptr) {}
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap), borrowed(o.borrowed) { o.p = nullptr; o.cap = 0; o.borrowed = false; }
    DevBuf& operator=(const DevBuf& o) { if (this != &o) { release(); p = o.p; cap = o.cap; borrowed = o.p != nullptr; } return *this; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) { release(); p = o.p; cap = o.cap; borrowed = o.borrowed; o.p = nullptr; o.cap = 0; o.borrowed = false; }
        return *this;
    }
    ~DevBuf() { release(); }
    int reserve(size_t bytes) {
        if (bytes <= cap) return 0;
        if (borrowed) return fail("internal: a buffer shared with the parent handle would have to grow");
        if (p) HIPCHK(hipFree(p));
        p = nullptr;
        cap = 0;
        size_t want = bytes + bytes / 8 + 256;
        if (hipError_t e = hipMalloc(&p, want); e != hipSuccess) {
            (void)hipGetLastError();
            p = nullptr;
            return fail("a device allocation of %zu bytes failed: %s", want, hipGetErrorString(e));
        }
        cap = want;
        return 0;
    }
    void release() {
        if (p && !borrowed) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        borrowed = false;
    }
    template <class T>
    T* as() const { return reinterpret_cast<T*>(p); }
};

// one packed Linear stack (lmi_set_mlp: the root, model 0; lmi_nav_set_model: an internal node's, model id >= 1)
struct Model {
    int n_layers = 0;
    std::vector<int> dims;    // dims[0..n_layers]
    std::vector<int> n_rb;    // per layer: output row-blocks
    std::vector<int> KG;      // per layer: k-groups of the layer's input
    std::vector<DevBuf> Wf;   // packed weights
    std::vector<DevBuf> bias; // padded bias
};

// ---- facts about the device (lmi_create) ----
struct DeviceFacts {
    int device = 0;
    int num_cus = 256;
    int scan_blocks_per_cu = 2;
    bool pf_hw_ok = false;       // fp16 subnormal self-test passed on this device
    double wall_khz = 100000.0;  // the chip's constant clock in kHz (device stamps)
    bool attrs16_done = false;   // storage16_kernel_attrs ran for this handle's device
};

// ---- what the caller set (lmi_subset hands them on) ----
struct Settings {
    int metric = 0;               // lmi_set_metric
    int storage_req = 0;          // lmi_set_storage: what the next lmi_buckets_begin builds (LMI_STORAGE_F32)
    bool prefilter = true;        // lmi_set_prefilter
    int fused_mlp = 1;            // lmi_set_fused_mlp: 0 never, 1 when the batch fills the chip, 2 always
    float stop_mass = 0.0f;       // lmi_set_stop_mass: 0 off; (0, 1]: a query's bucket order ends once this much probability is covered
    float path_mass = 0.0f;       // lmi_set_path_mass: 0 off; (0, 1]: a query's walk ends once its recorded buckets cover this much path probability
    int64_t stop_rows = 0;        // lmi_set_stop_rows: 0 off; > 0: a query's bucket order / walk ends once the buckets it has visited hold this many objects
    int timing_level = 2;         // lmi_set_timing
    bool chunk_rows_auto = true;  // until lmi_set_chunk_rows: lmi_buckets_begin picks 256..2048 by the index size
    int chunk_rows_set = 0;       // lmi_set_chunk_rows' value (a very large bucket raises chunk_rows above it; lmi_subset starts from it again)
};

// ---- developer switches: what lmi_create reads from the environment, and the test hook ----
struct Switches {
    int ps_force_wide = -1;        // LMI_PS_WIDE=0/1 pins it (developer aid)
    bool pf_small = true;          // d <= 128: pass2_small_kernel (LMI_PF_SMALL=0 in the environment: pass2_kernel for every d)
    bool pf_redo = true;           // overflow_rebound_kernel + pass 2's redo launch (LMI_PF_NO_REDO=1 in the environment: off)
    bool rescore_streamed = true;  // lmi_rescore.h (LMI_RESCORE_SIMPLE=1 in the environment: select_rescore_kernel)
    bool pf_qbound = true;         // LMI_PF_QBOUND=0: per-bucket bounds only (query_bound_kernel off)
    bool pf_primary = true;        // LMI_PF_PRIMARY=0: pass 1 samples every column although one bound per query is used
    bool debug_emit_all = false;   // lmi_debug_emit_all
    int use_tail = 1;              // tail_kernel (lmi_tail.h): selection + re-rank + rank merge in one wave per query (LMI_TAIL=0: the five launches of round 4;
                                   // 2: also group-wise for n_buckets > 4)
    bool graded_chunks = true;     // pass 2's items: chunk length per bucket and call (LMI_P2_GRADED=0: the index's static chunk everywhere)
    int chunk_lvl_rows[3] = {0, 0, 0};     // LMI_P2_CHUNKS=a,b,c (rows; 0 = 1, 1/2, 1/4 of the static chunk)
    float chunk_frac[2] = {0.16f, 0.05f};  // LMI_P2_CHUNK_FRAC=f0,f1: the last f0 of the work in chunks of b rows, the last f1 in chunks of c
    bool use_front = true;         // route_kernel + pack_kernel (lmi_front.h) instead of the eight preparation launches (LMI_FRONT=0 in the environment: off)
};

// ---- the navigation models and the tree (lmi_host_model.h, lmi_mlp_fused.h) ----
struct Models {
    std::vector<Model> models = std::vector<Model>(1);   // index = model id; models[0] is the root
    const Model& root() const { return models[0]; }
    bool desc_dirty = true;
    DevBuf d_models;                      // ModelDesc[models.size()]
    int fm_s0 = 0, fm_s1 = 0, fm_act0 = 0, fm_lds = 0, fm_logits_lds = 0;  // LDS plan of the current model set
    bool fm_ok = false;                   // every model fits the fused kernel
    // the tree: flat child index = child_offset[model] + class
    std::vector<int> h_child_offset, h_child_model, h_child_bucket;
    DevBuf d_child_offset, d_child_model, d_child_bucket;
    bool tree_set = false;
};

// ---- the bucket index: its shape, the host tables and every image on the device ----
struct Buckets {
    bool building = false, built = false;
    int64_t N = 0;
    int d = 0, L = 0, KGs = 0;     // d: dims of the STORED vectors (L2 metric: user dims + the norm column, padded to 4)
    int d_user = 0;                // dims of the caller's vectors
    int chunk_rows = 2048;
    int64_t n_rb_total = 0;
    std::vector<int> h_nb_rows, h_rb_start, h_nch;
    DevBuf slab, ids_slab, pos, d_nb_rows, d_rb_start, d_nch;
    int64_t rows_added = 0, owned_total = 0;
    bool indexed_ingest = false;  // lmi_buckets_add_owned_rows: only the owned objects are passed in
    // the fp16 prefilter's images (lmi_prefilter.h)
    bool have16 = false;     // slab16 built by lmi_buckets_end
    int KG16 = 0;
    int dp = 0;   // row pitch (floats) of `rowmajor` (LMI_STORAGE_F16: no such image; d rounded up to 8, the floats of a query the re-rank stages)
    int storage = 0;         // of the index being built / built (LMI_STORAGE_F32): LMI_STORAGE_F16 keeps slab16 only (lmi_store16.h)
    DevBuf slab16, rowmajor, xscale, xmaxbits, bnorm, bdelta;
    int n_nonempty = 1;      // buckets with rows, on any rank (lmi_buckets_begin)
    // mutation of a built index (lmi_buckets_insert / lmi_buckets_delete, lmi_mutate.h)
    std::vector<int> h_cap_rb;           // per bucket: row-blocks reserved at h_rb_start[b] (cdiv(n_b, 32) after a build)
    std::vector<unsigned char> h_owned;  // lmi_buckets_begin's `owned` (empty: every bucket)
    std::vector<unsigned char> h_any;    // per bucket: holds rows on some rank (n_nonempty)
    int64_t mut_paths[4] = {0, 0, 0, 0}; // lmi_debug_layout: buckets filled in their slack, buckets relocated, growth re-packs, hole re-packs
    // which layout this is (next_layout_stamp: lmi_buckets_end, every lmi_buckets_insert / _delete that changes the slab, lmi_subset's
    // output).  Copied with the struct: a clone view carries its parent's.  Read by the filters only (lmi_host_filter.h): a filter's
    // masks are keyed by slab position and hold for the handles that carry the stamp it was made under
    uint64_t layout_stamp = 0;
    // lmi_index_bytes: what is held for the index right now: the vector images, the ids, the per-bucket tables (a clone view: its parent's)
    int64_t index_bytes() const {
        int64_t t = 0;
        for (const DevBuf* x : {&slab, &slab16, &rowmajor, &ids_slab, &d_nb_rows, &d_rb_start, &d_nch, &xscale, &xmaxbits, &bnorm, &bdelta})
            t += x->p ? (int64_t)x->cap : 0;
        return t;
    }
};

struct lmi_index;

// a value no other layout of this process carries (never 0: a handle without a built index)
inline uint64_t next_layout_stamp() {
    static std::atomic<uint64_t> counter{0};
    return ++counter;
}

// ---- per handle: workspaces, staging, streams, events, timing and statistics.  Never copied: a clone view starts with a fresh one ----
struct CallState {
    CallState() = default;
    CallState(const CallState&) = delete;
    CallState& operator=(const CallState&) = delete;
    hipStream_t stream = nullptr;
    hipStream_t side = nullptr;           // library-owned: the per-layer MLP of a batch's tail beside the fused kernel (mlp_enqueue)
    hipEvent_t side_fork = nullptr, side_join = nullptr;
    DevBuf gather_send, gather_recv;      // lmi_allgather_merge
    DevBuf pq_prob, pq_ent, pq_len, nav_len, nav_slab, nav_ent, nav_count, nav_colq, nav_active;
    DevBuf pq_mass, nav_parent_mass, nav_cum;   // the path-mass stop: reserved only while it is on
    DevBuf nav_rows;                            // the row-budget stop of the walk ([nq] int64): reserved only while it is on
    DevBuf aug_rows, q_aug, qn2;   // L2: augmented ingest pieces / queries, |q|^2
    DevBuf stage;  // H2D staging for add_rows / host query uploads
    DevBuf wide;   // a piece of half rows widened to binary32 for an LMI_STORAGE_F32 build (the *_f16 ingest calls; widen16_kernel)
    DevBuf q16_nav, q16_srch;   // the uploaded halves of a host-pointer *_f16 search call, widened into q_nav / q_srch
    bool q_srch_async = false;  // an on_device *_f16 call widened into q_srch and did not synchronise: a later side-stream upload into
                                // q_srch (lmi_search_tree, host pointers) must wait for that call's scan first
    DevBuf rd_flag;             // lmi_bucket_read_f16 on an LMI_STORAGE_F32 index: [0] != 0 -> a value was not binary16-exact
    DevBuf qdelta, qnorm, qscale, qfrag16, eps2, cand_cnt, cand_row, cand_s, fallback, pf_bound, nkeep, surv_row, rs_flag, rs_active;
    DevBuf grp_scratch;      // route_group_kernel<true>: the bucket sort of fan-outs past ROUTE_MAX_BUCKETS
    DevBuf x_log, x_ext, x_off, fb_list;  // the candidates' overflow log, its by-column sorted form and offsets (lmi_prefilter.h, OverflowLog);
                                          // the fallback list: [count, fail0, fail1, log head, sorted total, pad x 3 | nslots slots]
    unsigned x_cap = 0;                   // entries of the log (0: not allocated yet)
    DevBuf redo;   // [1] count | [L] bucket flags | [columns] column flags (bytes): overflow_rebound_kernel
    size_t stamps_off = 0;         // developer builds: byte offset of the phase stamps inside pf_bound
    int last_nslots = 0, last_nb = 0;
    long long last_ncols = 0;
    bool last_fast = false;
    static constexpr int PLAN_WORDS = 32;
    int32_t last_plan[PLAN_WORDS] = {};   // lmi_debug_last_plan: the LMI_PLAN_* words of the last scan, written by scan_enqueue and its launch sites
    int32_t last_mlp_plan[PLAN_WORDS] = {};   // lmi_debug_last_mlp_plan: the LMI_MLP_PLAN_* words of the last MLP forward, written by mlp_enqueue and its launch sites
    DevBuf act[2], xfrag, logits, order, q_nav, q_srch;
    DevBuf m, cb_start, item_base, part_base, stats, head, slot_local, slot_col, colmap, qfrag, grp, col_thr;
    DevBuf part_score, part_row, rank_d, rank_id, out_d, out_id, out_key;
    // hipEvents of the last EV_RING calls: lmi_timings reads the newest set, lmi_timings_mean averages all
    // sets since lmi_timings_reset with ONE stream synchronisation (no per-call sync in a timed loop)
    static constexpr int EV_RING = 128;
    hipEvent_t ev_ring[EV_RING][10] = {};
    bool valid_ring[EV_RING][10] = {};
    int ev_cur = 0;
    long long ev_calls = 0;  // calls since lmi_timings_reset
    hipEvent_t* ev = ev_ring[0];
    bool* ev_valid = valid_ring[0];
    long long h_stats[4] = {0, 0, 0, 0};
    bool stats_pending = false;
    // device-side phase stamps (timing level 2; lmi_kernels.h): a ring of EV_RING sets of ST_COUNT words, the set of the current
    // call, which of its stamps a kernel of the call was given (host-side mask)
    DevBuf ts_ring;
    unsigned ts_mask[EV_RING] = {};
    unsigned long long* ts_set = nullptr;
    DevBuf fr_dbg;                // LMI_FR_DEBUG=1: route_kernel's / pack_kernel's phase stamps (lmi_debug_peek "fr_dbg")
    DevBuf cb_alloc, cb_bucket;   // lmi_front.h: the call-tagged granules of route_kernel (zero at allocation) and the col-blocks' buckets
    unsigned* h_oflag = nullptr;  // a word of pinned host memory (device-visible): "the last batch used the overflow log" (RescoreParams::host_oflag)
    int overflow_armed = 0;       // calls for which overflow_rebound_kernel + pass 2's redo launch stay in the sequence (re-armed by h_oflag)
    bool fr_bump_pending = false; // route_kernel was launched and the launch that bumps the granules' tag (bound_merge2_kernel) not yet: a call that
                                  // failed in between is repaired by a bump launch of its own at the next call
    DevBuf mut_pos, mut_ids, mut_list, mut_keep, mut_src, mut_stage, mut_word;   // a mutation's / lmi_subset's maps
    lmi_index* parent = nullptr;  // a clone view: the handle whose memory it borrows
    int live_clones = 0;          // clone views of this handle that are alive (a mutation is refused while any is)
};

struct lmi_index : DeviceFacts, Settings, Switches, Models, Buckets, CallState {};

// A clone view of h (lmi_clone_view): the device facts, settings and switches are copies; the models and the bucket index are copies
// whose every DevBuf is a borrowed view of h's memory (tables by value); the call state is its own, fresh.  No HIP call.
static lmi_index* clone_handle(lmi_index* h) {
    lmi_index* c = new lmi_index();
    static_cast<DeviceFacts&>(*c) = *h;
    static_cast<Settings&>(*c) = *h;
    static_cast<Switches&>(*c) = *h;
    static_cast<Models&>(*c) = *h;
    static_cast<Buckets&>(*c) = *h;
    c->parent = h;   // lmi_buckets_insert / _delete refuse to run on h while c lives (c copied h's bucket tables)
    h->live_clones++;
    return c;
}
