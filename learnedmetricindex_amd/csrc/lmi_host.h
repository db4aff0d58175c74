// lmi_host.h -- what every host-side header shares: error reporting, the growing device buffer, the handle (lmi_index) and the
// per-call helpers (timing events and device stamps, input staging, the library's side stream).
#pragma once
#include "lmi_kernels.h"
#include "lmi_prefilter.h"
#include "lmi_pass2.h"
#include "lmi_pass2_small.h"
#include "lmi_mlp_fused.h"
#include "lmi_rescore.h"
#include "lmi_front.h"
#include "lmi_tail.h"
#include "lmi_mutate.h"
#include "lmi_store16.h"

#include <algorithm>
#include <cfloat>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "lmi_hip.h"

using namespace lmi;

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

inline int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }
inline long long rup(long long a, long long b) { return (a + b - 1) / b * b; }

// device buffer that only grows
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    bool borrowed = false;  // lmi_clone_view: the memory belongs to the handle this one was cloned from
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
    void borrow() { borrowed = p != nullptr; }   // keep the pointer, never free it
    void forget() { p = nullptr; cap = 0; borrowed = false; }  // a copied struct's workspace: start empty
    template <class T>
    T* as() const { return reinterpret_cast<T*>(p); }
};

}  // namespace

struct lmi_index {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t side = nullptr;           // library-owned: the per-layer MLP of a batch's tail beside the fused kernel (mlp_enqueue)
    hipEvent_t side_fork = nullptr, side_join = nullptr;
    int num_cus = 256;
    int scan_blocks_per_cu = 2;

    // ---- MLP ----
    int n_layers = 0;
    std::vector<int> dims;    // dims[0..n_layers]
    std::vector<int> n_rb;    // per layer: output row-blocks
    std::vector<int> KG;      // per layer: k-groups of the layer's input
    std::vector<DevBuf> Wf;   // packed weights
    std::vector<DevBuf> bias; // padded bias

    // ---- fused MLP / multi-level navigation (lmi_mlp_fused.h) ----
    struct NodeModel {            // an internal node's model (model id >= 1; the root is the fields above)
        int n_layers = 0;
        std::vector<int> dims, n_rb, KG;
        std::vector<DevBuf> Wf, bias;
    };
    std::vector<NodeModel> node_models;   // index = model id - 1
    int fused_mlp = 1;                    // lmi_set_fused_mlp: 0 never, 1 when the batch fills the chip, 2 always
    float stop_mass = 0.0f;               // lmi_set_stop_mass: 0 off; (0, 1]: a query's bucket order ends once this much probability is covered
    float path_mass = 0.0f;               // lmi_set_path_mass: 0 off; (0, 1]: a query's walk ends once its recorded buckets cover this much path probability
    bool desc_dirty = true;
    DevBuf d_models;                      // ModelDesc[1 + node_models.size()]
    int fm_s0 = 0, fm_s1 = 0, fm_act0 = 0, fm_lds = 0, fm_logits_lds = 0;  // LDS plan of the current model set
    bool fm_ok = false;                   // every model fits the fused kernel
    // the tree: flat child index = child_offset[model] + class
    std::vector<int> h_child_offset, h_child_model, h_child_bucket;
    DevBuf d_child_offset, d_child_model, d_child_bucket;
    bool tree_set = false;
    DevBuf gather_send, gather_recv;      // lmi_allgather_merge
    DevBuf pq_prob, pq_ent, pq_len, nav_len, nav_slab, nav_ent, nav_count, nav_colq, nav_active;
    DevBuf pq_mass, nav_parent_mass, nav_cum;   // the path-mass stop: reserved only while it is on

    // ---- buckets ----
    bool building = false, built = false;
    int64_t N = 0;
    int d = 0, L = 0, KGs = 0;     // d: dims of the STORED vectors (L2 metric: user dims + the norm column, padded to 4)
    int metric = 0, d_user = 0;    // lmi_set_metric; dims of the caller's vectors
    DevBuf aug_rows, q_aug, qn2;   // L2: augmented ingest pieces / queries, |q|^2
    int chunk_rows = 2048;
    bool chunk_rows_auto = true;  // until lmi_set_chunk_rows: lmi_buckets_begin picks 256..2048 by the index size
    int chunk_rows_set = 0;       // lmi_set_chunk_rows' value (a very large bucket raises chunk_rows above it; lmi_subset starts from it again)
    int64_t n_rb_total = 0;
    std::vector<int> h_nb_rows, h_rb_start, h_nch;
    DevBuf slab, ids_slab, pos, d_nb_rows, d_rb_start, d_nch;
    int64_t rows_added = 0, owned_total = 0;
    bool indexed_ingest = false;  // lmi_buckets_add_owned_rows: only the owned objects are passed in
    DevBuf stage;  // H2D staging for add_rows / host query uploads
    DevBuf wide;   // a piece of half rows widened to binary32 for an LMI_STORAGE_F32 build (the *_f16 ingest calls; widen16_kernel)
    DevBuf q16_nav, q16_srch;   // the uploaded halves of a host-pointer *_f16 search call, widened into q_nav / q_srch
    bool q_srch_async = false;  // an on_device *_f16 call widened into q_srch and did not synchronise: a later side-stream upload into
                                // q_srch (lmi_search_tree, host pointers) must wait for that call's scan first
    DevBuf rd_flag;             // lmi_bucket_read_f16 on an LMI_STORAGE_F32 index: [0] != 0 -> a value was not binary16-exact
    // ---- fp16 prefilter (lmi_prefilter.h) ----
    bool prefilter = true;   // lmi_set_prefilter
    bool pf_hw_ok = false;   // fp16 subnormal self-test passed on this device
    bool have16 = false;     // slab16 built by lmi_buckets_end
    int KG16 = 0;
    int dp = 0;   // row pitch (floats) of `rowmajor` (LMI_STORAGE_F16: no such image; d rounded up to 8, the floats of a query the re-rank stages)
    int storage = LMI_STORAGE_F32;       // of the index being built / built: LMI_STORAGE_F16 keeps slab16 only (lmi_store16.h)
    int storage_req = LMI_STORAGE_F32;   // lmi_set_storage: what the next lmi_buckets_begin builds
    bool attrs16_done = false;           // storage16_kernel_attrs ran for this handle's device
    DevBuf slab16, rowmajor, xscale, xmaxbits, bnorm, bdelta, qdelta;
    DevBuf qnorm, qscale, qfrag16, eps2, cand_cnt, cand_row, cand_s, fallback, pf_bound, nkeep, surv_row, rs_flag, rs_active;
    DevBuf grp_scratch;      // route_group_kernel<true>: the bucket sort of fan-outs past ROUTE_MAX_BUCKETS
    int ps_force_wide = -1;  // LMI_PS_WIDE=0/1 pins it (developer aid)
    int n_nonempty = 1;      // buckets with rows, on any rank (lmi_buckets_begin)
    DevBuf x_log, x_ext, x_off, fb_list;  // the candidates' overflow log, its by-column sorted form and offsets (lmi_prefilter.h, OverflowLog);
                                          // the fallback list: [count, fail0, fail1, log head, sorted total, pad x 3 | nslots slots]
    unsigned x_cap = 0;                   // entries of the log (0: not allocated yet)
    DevBuf redo;   // [1] count | [L] bucket flags | [columns] column flags (bytes): overflow_rebound_kernel
    size_t stamps_off = 0;         // developer builds: byte offset of the phase stamps inside pf_bound
    bool pf_small = true;          // d <= 128: pass2_small_kernel (LMI_PF_SMALL=0 in the environment: pass2_kernel for every d)
    bool pf_redo = true;           // overflow_rebound_kernel + pass 2's redo launch (LMI_PF_NO_REDO=1 in the environment: off)
    bool rescore_streamed = true;  // lmi_rescore.h (LMI_RESCORE_SIMPLE=1 in the environment: select_rescore_kernel)
    int last_nslots = 0, last_nb = 0;
    long long last_ncols = 0;
    bool last_fast = false;
    bool pf_qbound = true;        // LMI_PF_QBOUND=0: per-bucket bounds only (query_bound_kernel off)
    bool pf_primary = true;       // LMI_PF_PRIMARY=0: pass 1 samples every column although one bound per query is used
    bool debug_emit_all = false;  // lmi_debug_emit_all

    // ---- per-call workspaces ----
    DevBuf act[2], xfrag, logits, order, q_nav, q_srch;
    DevBuf m, cb_start, item_base, part_base, stats, head, slot_local, slot_col, colmap, qfrag, grp, col_thr;
    DevBuf part_score, part_row, rank_d, rank_id, out_d, out_id, out_key;
    // hipEvents of the last EV_RING calls: lmi_timings reads the newest set, lmi_timings_mean averages all
    // sets since lmi_timings_reset with ONE stream synchronisation (no per-call sync in a timed loop)
    static constexpr int EV_RING = 128;
    hipEvent_t ev_ring[EV_RING][10] = {};
    bool valid_ring[EV_RING][10] = {};
    int ev_cur = 0;
    int timing_level = 2;  // lmi_set_timing
    long long ev_calls = 0;  // calls since lmi_timings_reset
    hipEvent_t* ev = ev_ring[0];
    bool* ev_valid = valid_ring[0];
    long long h_stats[4] = {0, 0, 0, 0};
    bool stats_pending = false;
    // device-side phase stamps (timing level 2; lmi_kernels.h): a ring of EV_RING sets of ST_COUNT words, the set of the current
    // call, which of its stamps a kernel of the call was given (host-side mask), the chip's constant clock in kHz
    DevBuf ts_ring;
    unsigned ts_mask[EV_RING] = {};
    unsigned long long* ts_set = nullptr;
    double wall_khz = 100000.0;
    DevBuf fr_dbg;                // LMI_FR_DEBUG=1: route_kernel's / pack_kernel's phase stamps (lmi_debug_peek "fr_dbg")
    DevBuf cb_alloc, cb_bucket;   // lmi_front.h: the call-tagged granules of route_kernel (zero at allocation) and the col-blocks' buckets
    unsigned* h_oflag = nullptr;  // a word of pinned host memory (device-visible): "the last batch used the overflow log" (RescoreParams::host_oflag)
    int overflow_armed = 0;       // calls for which overflow_rebound_kernel + pass 2's redo launch stay in the sequence (re-armed by h_oflag)
    bool fr_bump_pending = false; // route_kernel was launched and the launch that bumps the granules' tag (bound_merge2_kernel) not yet: a call that
                                  // failed in between is repaired by a bump launch of its own at the next call
    int use_tail = 1;             // tail_kernel (lmi_tail.h): selection + re-rank + rank merge in one wave per query (LMI_TAIL=0: the five launches of round 4;
                                  // 2: also group-wise for n_buckets > 4)
    bool graded_chunks = true;    // pass 2's items: chunk length per bucket and call (LMI_P2_GRADED=0: the index's static chunk everywhere)
    int chunk_lvl_rows[3] = {0, 0, 0};   // LMI_P2_CHUNKS=a,b,c (rows; 0 = 1, 1/2, 1/4 of the static chunk)
    float chunk_frac[2] = {0.16f, 0.05f};   // LMI_P2_CHUNK_FRAC=f0,f1: the last f0 of the work in chunks of b rows, the last f1 in chunks of c
    bool use_front = true;        // route_kernel + pack_kernel (lmi_front.h) instead of the eight preparation launches (LMI_FRONT=0 in the environment: off)

    // ---- mutation of a built index (lmi_buckets_insert / lmi_buckets_delete, lmi_mutate.h) ----
    std::vector<int> h_cap_rb;           // per bucket: row-blocks reserved at h_rb_start[b] (cdiv(n_b, 32) after a build)
    std::vector<unsigned char> h_owned;  // lmi_buckets_begin's `owned` (empty: every bucket)
    std::vector<unsigned char> h_any;    // per bucket: holds rows on some rank (n_nonempty)
    lmi_index* parent = nullptr;         // a clone view: the handle whose memory it borrows
    int live_clones = 0;                 // clone views of this handle that are alive (a mutation is refused while any is)
    int64_t mut_paths[4] = {0, 0, 0, 0}; // lmi_debug_layout: buckets filled in their slack, buckets relocated, growth re-packs, hole re-packs
    DevBuf mut_pos, mut_ids, mut_list, mut_keep, mut_src, mut_stage, mut_word;
};

// The handle's device buffers, each listed once.  each_index_buf: the index and the models' tables -- what a clone view borrows from
// its parent; each_call_buf: workspaces, staging and timing buffers -- every handle's own.  (The models' weights: vectors of their own.)
template <class F>
static void each_index_buf(lmi_index* h, F f) {
    DevBuf* b[] = {&h->d_models, &h->d_child_offset, &h->d_child_model, &h->d_child_bucket, &h->slab, &h->ids_slab, &h->pos, &h->d_nb_rows,
                   &h->d_rb_start, &h->d_nch, &h->slab16, &h->rowmajor, &h->xscale, &h->xmaxbits, &h->bnorm, &h->bdelta};
    for (DevBuf* x : b) f(*x);
}
template <class F>
static void each_call_buf(lmi_index* h, F f) {
    DevBuf* b[] = {&h->gather_send, &h->gather_recv, &h->pq_prob, &h->pq_ent, &h->pq_len, &h->nav_len, &h->nav_slab, &h->nav_ent, &h->nav_count,
                   &h->nav_colq, &h->nav_active, &h->pq_mass, &h->nav_parent_mass, &h->nav_cum, &h->aug_rows, &h->q_aug, &h->qn2, &h->stage, &h->wide, &h->q16_nav, &h->q16_srch, &h->rd_flag, &h->qdelta, &h->qnorm, &h->qscale, &h->qfrag16,
                   &h->eps2, &h->cand_cnt, &h->cand_row, &h->cand_s, &h->fallback, &h->pf_bound, &h->nkeep, &h->redo, &h->surv_row, &h->rs_flag,
                   &h->rs_active, &h->act[0], &h->act[1], &h->xfrag, &h->logits, &h->order, &h->q_nav, &h->q_srch, &h->m, &h->cb_start,
                   &h->item_base, &h->part_base, &h->stats, &h->head, &h->slot_local, &h->slot_col, &h->colmap, &h->qfrag, &h->grp, &h->col_thr,
                   &h->part_score, &h->part_row, &h->rank_d, &h->rank_id, &h->out_d, &h->out_id, &h->out_key, &h->x_log, &h->x_ext, &h->x_off,
                   &h->fb_list, &h->grp_scratch, &h->ts_ring, &h->fr_dbg, &h->cb_alloc, &h->cb_bucket, &h->mut_pos, &h->mut_ids, &h->mut_list,
                   &h->mut_keep, &h->mut_src, &h->mut_stage, &h->mut_word};
    for (DevBuf* x : b) f(*x);
}

// the low-dimensional form of the prefilter (d <= 128: lmi_pass2_small.h) for an index of kg16 k16-groups; otherwise pass2_kernel
static bool low_d_form(const lmi_index* h, int kg16) { return h->pf_small && kg16 <= PS_MAXKG; }
// which fp16 fragment shape the index and the queries are packed in: 16 x 32 for pass2_kernel, 32 x 16 for the low-dimensional kernels
static int frag16x16(const lmi_index* h) { return low_d_form(h, h->KG16) ? 0 : 1; }

// why an LMI_STORAGE_F16 build cannot go with the handle's other settings (nullptr: it can)
static const char* storage16_conflict(const lmi_index* h) {
    if (!h->pf_hw_ok) return "the fp16 subnormal self-test failed on this device: the fp16 fragments cannot be trusted to hold the vectors";
    if (h->metric == LMI_METRIC_L2) return "LMI_METRIC_L2 is not supported (the -|x|^2/2 column of a stored vector is not fp16-exact)";
    if (!h->prefilter) return "lmi_set_prefilter(0) is not supported (the all-f32 scan needs f32 fragments)";
    return nullptr;
}

// the dynamic-LDS limits of the re-rank kernels' LMI_STORAGE_F16 forms: set when a handle first builds such an index (per device;
// handles that never do -- lmi_knn_ip's among them -- do not pay for it)
static int storage16_kernel_attrs(lmi_index* h) {
    if (h->attrs16_done) return 0;
#define LMI_RC16_ATTR(GV) \
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&rescore_kernel<GV, false, true, Frag16>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)); \
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&rescore_kernel<GV, true, true, Frag16>), hipFuncAttributeMaxDynamicSharedMemorySize, RC_SMALL_LDS_CAP)); \
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&tail_kernel<GV, true, Frag16>), hipFuncAttributeMaxDynamicSharedMemorySize, RC_SMALL_LDS_CAP));
    LMI_RC16_ATTR(1) LMI_RC16_ATTR(2) LMI_RC16_ATTR(3) LMI_RC16_ATTR(4)
#undef LMI_RC16_ATTR
    h->attrs16_done = true;
    return 0;
}

static int set_dev(lmi_index* h) {
    HIPCHK(hipSetDevice(h->device));
    return 0;
}

// ---- per call: the timing ring, device stamps, input staging, the side stream ----
static void begin_call(lmi_index* h) {
    h->ev_cur = (h->ev_cur + 1) % lmi_index::EV_RING;
    h->ev = h->ev_ring[h->ev_cur];
    h->ev_valid = h->valid_ring[h->ev_cur];
    for (int i = 0; i < 10; ++i) h->ev_valid[i] = false;
    ++h->ev_calls;
    h->ts_mask[h->ev_cur] = 0u;
    h->ts_set = nullptr;
    if (h->timing_level == 2) {   // device stamps: the call's set of the ring (allocated with the first timed call; a failed allocation: no stamps)
        if (!h->ts_ring.p && h->ts_ring.reserve((size_t)lmi_index::EV_RING * ST_COUNT * 8) != 0) return;
        h->ts_set = h->ts_ring.as<unsigned long long>() + (size_t)h->ev_cur * ST_COUNT;
    }
}
// the device word a kernel of this call writes stamp `idx` to (nullptr: stamps are off)
static unsigned long long* tsp(lmi_index* h, int idx) {
    if (!h->ts_set) return nullptr;
    h->ts_mask[h->ev_cur] |= 1u << idx;
    return h->ts_set + idx;
}
// the end of a call whose last kernel carries no stamp (lmi_mlp_topk, lmi_nav_order ..): one single-thread launch behind it
static int stamp_end(lmi_index* h, int idx) {
    if (unsigned long long* p = tsp(h, idx)) {
        stamp_kernel<<<1, 1, 0, h->stream>>>(p);
        HIPCHK(hipGetLastError());
    }
    return 0;
}

static int record(lmi_index* h, int i) {
    // every recorded event is a ~5 us bubble between two kernels: level 3 records every phase boundary, level 1 the call's first
    // and last event (LMI_T_TOTAL), levels 0 and 2 none (2: the kernels stamp the chip's clock themselves, tsp)
    if (h->timing_level == 0 || h->timing_level == 2 || (h->timing_level == 1 && i != 0 && i != 1 && i != 4)) return 0;
    if (!h->ev[i]) HIPCHK(hipEventCreateWithFlags(&h->ev[i], hipEventDisableSystemFence));   // timing only: no system-scope release at the record
    HIPCHK(hipEventRecord(h->ev[i], h->stream));
    h->ev_valid[i] = true;
    return 0;
}

// device pointer to the caller's input (uploads host data into `buf`)
static int input_ptr(lmi_index* h, const void* src, size_t bytes, int on_device, DevBuf& buf, const void** out) {
    if (on_device) { *out = src; return 0; }
    CHK(buf.reserve(bytes));
    HIPCHK(hipMemcpyAsync(buf.p, src, bytes, hipMemcpyHostToDevice, h->stream));
    *out = buf.p;
    return 0;
}

// Binary16 sources (halves as uint16 bit patterns; a caller's pointer is only 2-byte aligned): a kernel may read 8 halves with one
// 16-byte load only where d % 8 == 0 and the base is 16-byte aligned -- then every row starts on a 16-byte boundary.  Per launch.
static bool half_src_vec(const void* src, int d) { return d % 8 == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0; }
// n rows of d halves at `src` (device) -> binary32 at `dst` (a buffer of the library's: 16-byte aligned), on stream s
static int widen16_enqueue(const void* src, long long n, int d, float* dst, hipStream_t s) {
    const long long total = n * d;
    if (total == 0) return 0;
    if (half_src_vec(src, d)) widen16_kernel<true><<<cdiv(total >> 3, 256), 256, 0, s>>>(static_cast<const unsigned short*>(src), total, dst);
    else widen16_kernel<false><<<cdiv(total, 256), 256, 0, s>>>(static_cast<const unsigned short*>(src), total, dst);
    HIPCHK(hipGetLastError());
    return 0;
}
// device pointer to the binary32 form of a half input of n rows x d: the halves are uploaded (host data; half the bytes) into `raw` and
// widened into `buf`, the handle's buffer for that input; a device pointer is widened from where it lies (the caller's memory is only read)
static int input_ptr16(lmi_index* h, const void* src, long long n, int d, int on_device, DevBuf& raw, DevBuf& buf, const void** out) {
    CHK(buf.reserve((size_t)n * d * 4));
    if (!on_device) {
        CHK(raw.reserve((size_t)n * d * 2));
        HIPCHK(hipMemcpyAsync(raw.p, src, (size_t)n * d * 2, hipMemcpyHostToDevice, h->stream));
        src = raw.p;
    }
    else if (&buf == &h->q_srch) h->q_srch_async = true;
    CHK(widen16_enqueue(src, n, d, buf.as<float>(), h->stream));
    *out = buf.p;
    return 0;
}

// the end of a host-pointer call: the listed device arrays back to the caller's, on h->stream in the order given, then the
// synchronisation.  An entry whose host pointer is null is skipped: that is how optional outputs (keys, logits, the bucket order of
// a search) are declined, and a required output passed as null (never valid) is now skipped too, not handed to the copy
struct HostCopy { void* host; const void* dev; size_t bytes; };
static int copy_back(lmi_index* h, std::initializer_list<HostCopy> list) {
    for (const HostCopy& c : list)
        if (c.host) HIPCHK(hipMemcpyAsync(c.host, c.dev, c.bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

// Side stream (library-owned): work that does not depend on what the handle's stream runs next is forked onto it and
// joined before its results are needed.  side_fork: the side stream waits for everything enqueued on h->stream so far.
static int side_ensure(lmi_index* h) {
    if (!h->side) {
        HIPCHK(hipStreamCreateWithFlags(&h->side, hipStreamNonBlocking));
        HIPCHK(hipEventCreateWithFlags(&h->side_fork, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&h->side_join, hipEventDisableTiming));
    }
    return 0;
}
static int side_fork(lmi_index* h) {
    CHK(side_ensure(h));
    HIPCHK(hipEventRecord(h->side_fork, h->stream));
    HIPCHK(hipStreamWaitEvent(h->side, h->side_fork, 0));
    return 0;
}
static int side_join(lmi_index* h) {
    HIPCHK(hipEventRecord(h->side_join, h->side));
    HIPCHK(hipStreamWaitEvent(h->stream, h->side_join, 0));
    return 0;
}
