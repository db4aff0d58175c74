// handle_selftest.cpp -- the ownership rules of csrc/lmi_handle.h, checked on the CPU: DevBuf (copy borrows, move hands on, the
// destructor frees) and the handle's parts (what clone_handle shares, what it leaves fresh, who frees what).  Stand-alone: the four
// HIP calls DevBuf makes are defined here over malloc / free with a record of the live allocations, no HIP library is linked.  Built
// with -fsanitize=address,undefined and leak detection by tests/test_handle_host.py.
#include "lmi_handle.h"

#include <cstdlib>
#include <cstring>
#include <set>
#include <type_traits>

static std::set<void*> g_live;     // what hipMalloc handed out and hipFree has not taken back
static bool g_fail_next = false;   // the next hipMalloc fails
extern "C" hipError_t hipMalloc(void** p, size_t n) {
    if (g_fail_next) { g_fail_next = false; *p = nullptr; return hipErrorOutOfMemory; }
    *p = malloc(n);
    if (!*p) return hipErrorOutOfMemory;
    g_live.insert(*p);
    return hipSuccess;
}
extern "C" hipError_t hipFree(void* p) {
    if (!g_live.erase(p)) { fprintf(stderr, "hipFree(%p): not a live allocation (freed twice, or never made)\n", p); abort(); }
    free(p);
    return hipSuccess;
}
extern "C" hipError_t hipGetLastError(void) { return hipSuccess; }
extern "C" const char* hipGetErrorString(hipError_t) { return "selftest error"; }

#define REQUIRE(cond)                                                                          \
    do {                                                                                       \
        if (!(cond)) { fprintf(stderr, "%s:%d: REQUIRE(%s) failed\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

static bool empty(const DevBuf& b) { return !b.p && b.cap == 0 && !b.borrowed; }
static bool view_of(const DevBuf& v, const DevBuf& owner) { return v.p && v.p == owner.p && v.cap == owner.cap && v.borrowed && !owner.borrowed; }

// an error in the middle of a function: the second allocation fails, CHK returns, the first temporary must not leak
static int error_path() {
    DevBuf a, b;
    CHK(a.reserve(1000));
    g_fail_next = true;
    CHK(b.reserve(1000));
    return 0;
}

static void devbuf_rules() {
    REQUIRE(empty(DevBuf()));
    {
        DevBuf a;
        REQUIRE(a.reserve(100) == 0 && a.p && a.cap >= 100 && !a.borrowed && g_live.size() == 1);
        void* const p = a.p;
        REQUIRE(a.reserve(50) == 0 && a.p == p);   // only grows
        {   // the copy borrows: same memory, cannot grow, frees nothing
            DevBuf v(a), w;
            w = a;
            REQUIRE(view_of(v, a) && view_of(w, a));
            REQUIRE(v.reserve(a.cap) == 0 && v.p == p);
            REQUIRE(v.reserve(a.cap + 1) != 0 && g_err.find("would have to grow") != std::string::npos && view_of(v, a));
            DevBuf vv(v);                       // a view's copy is a view
            REQUIRE(view_of(vv, a));
            w.release();
            REQUIRE(empty(w) && g_live.size() == 1);
            DevBuf e, ee(e);                    // an empty buffer's copy is empty and may grow
            REQUIRE(empty(ee) && ee.reserve(10) == 0 && !ee.borrowed && g_live.size() == 2);
        }
        REQUIRE(g_live.size() == 1 && g_live.count(p));
        DevBuf m(std::move(a));                 // the move hands the memory on
        REQUIRE(empty(a) && m.p == p && !m.borrowed && g_live.size() == 1);
        DevBuf n;
        REQUIRE(n.reserve(10) == 0 && g_live.size() == 2);
        n = std::move(m);                       // ... and frees what the target held
        REQUIRE(empty(m) && n.p == p && !n.borrowed && g_live.size() == 1);
        n = std::move(*&n);                     // onto itself: nothing happens
        REQUIRE(n.p == p && g_live.size() == 1);
    }
    REQUIRE(g_live.empty());                    // the destructor freed it
    {   // a vector that grows moves its elements: the three allocations stay what they were
        static_assert(std::is_nothrow_move_constructible<DevBuf>::value && std::is_nothrow_move_assignable<DevBuf>::value, "vector<DevBuf> must move");
        std::vector<DevBuf> v(3);
        void* p[3];
        for (int i = 0; i < 3; ++i) { REQUIRE(v[i].reserve(64 + i) == 0); p[i] = v[i].p; }
        v.resize(50);
        for (int i = 0; i < 3; ++i) REQUIRE(v[i].p == p[i] && !v[i].borrowed && g_live.count(p[i]));
        for (int i = 3; i < 50; ++i) REQUIRE(empty(v[i]));
        REQUIRE(g_live.size() == 3);
        std::vector<DevBuf> views = v;          // a copied vector: views
        for (int i = 0; i < 3; ++i) REQUIRE(view_of(views[i], v[i]));
    }
    REQUIRE(g_live.empty());
    REQUIRE(error_path() != 0 && g_err.find("a device allocation of") != std::string::npos);
    REQUIRE(g_live.empty());
}

// ---- the handle ----
static DevBuf Models::* const kModelBufs[] = {&Models::d_models, &Models::d_child_offset, &Models::d_child_model, &Models::d_child_bucket};
static DevBuf Buckets::* const kImages[] = {&Buckets::slab,   &Buckets::ids_slab, &Buckets::pos,    &Buckets::d_nb_rows, &Buckets::d_rb_start, &Buckets::d_nch,
                                            &Buckets::slab16, &Buckets::rowmajor, &Buckets::xscale, &Buckets::xmaxbits,  &Buckets::bnorm,      &Buckets::bdelta};
static DevBuf CallState::* const kWork[] = {&CallState::stage,    &CallState::q_nav,   &CallState::q_srch,   &CallState::logits,  &CallState::order,
                                            &CallState::cand_row, &CallState::pf_bound, &CallState::ts_ring, &CallState::cb_alloc, &CallState::mut_keep,
                                            &CallState::out_d,    &CallState::gather_send, &CallState::nav_slab, &CallState::x_log};

static void reserve_work(lmi_index* h) {
    for (auto m : kWork) REQUIRE((h->*m).reserve(512) == 0);
    REQUIRE(h->act[0].reserve(512) == 0 && h->act[1].reserve(512) == 0);
}

static lmi_index* make_parent() {
    lmi_index* h = new lmi_index();
    h->device = 3; h->num_cus = 64; h->scan_blocks_per_cu = 1; h->pf_hw_ok = true; h->wall_khz = 5.0; h->attrs16_done = true;
    h->metric = 1; h->storage_req = 1; h->prefilter = false; h->fused_mlp = 2; h->stop_mass = 0.5f; h->path_mass = 0.25f;
    h->timing_level = 3; h->chunk_rows_auto = false; h->chunk_rows_set = 512;
    h->ps_force_wide = 1; h->pf_small = false; h->pf_redo = false; h->rescore_streamed = false; h->pf_qbound = false; h->pf_primary = false;
    h->debug_emit_all = true; h->use_tail = 2; h->graded_chunks = false; h->chunk_lvl_rows[1] = 7; h->chunk_frac[1] = 0.5f; h->use_front = false;
    h->models.resize(3);   // the root and two nodes
    for (Model& m : h->models) {
        m.dims = {8, 40, 4}; m.n_rb = {2, 1}; m.KG = {1, 8};
        m.Wf.assign(2, DevBuf()); m.bias.assign(2, DevBuf());
        for (int i = 0; i < 2; ++i) REQUIRE(m.Wf[i].reserve(2048) == 0 && m.bias[i].reserve(128) == 0);
        m.n_layers = 2;
    }
    h->h_child_offset = {0, 4, 8, 12}; h->h_child_model.assign(12, -1); h->h_child_bucket.assign(12, 0);
    for (auto m : kModelBufs) REQUIRE((h->*m).reserve(64) == 0);
    h->tree_set = true; h->desc_dirty = false; h->fm_ok = true; h->fm_lds = 4096;
    h->built = true; h->N = 100; h->d = 16; h->L = 4; h->KGs = 2; h->d_user = 15; h->chunk_rows = 512; h->n_rb_total = 5;
    h->h_nb_rows = {10, 20, 30, 40}; h->h_rb_start = {0, 1, 2, 3, 5}; h->h_nch = {1, 1, 1, 1}; h->h_cap_rb = {1, 1, 1, 2};
    h->h_any = {1, 1, 1, 1}; h->have16 = true; h->KG16 = 1; h->dp = 16; h->storage = 1; h->rows_added = 100; h->owned_total = 100;
    for (int i = 0; i < 4; ++i) h->mut_paths[i] = 11 + i;
    for (auto m : kImages) REQUIRE((h->*m).reserve(1024) == 0);
    reserve_work(h);
    // a call state that has been used: none of it may show in a clone
    h->q_srch_async = true; h->fr_bump_pending = true; h->stats_pending = true; h->x_cap = 99; h->overflow_armed = 5; h->stamps_off = 64;
    h->last_nslots = 256; h->last_nb = 4; h->last_ncols = 64; h->last_fast = true; h->ev_cur = 5; h->ev_calls = 6;
    for (int i = 0; i < CallState::PLAN_WORDS; ++i) h->last_plan[i] = 1 + i;
    h->ev = h->ev_ring[5]; h->ev_valid = h->valid_ring[5]; h->valid_ring[5][0] = true; h->ts_mask[5] = 7u;
    h->ts_set = h->ts_ring.as<unsigned long long>();
    for (int i = 0; i < 4; ++i) h->h_stats[i] = 1000 + i;
    return h;
}

static bool same(const DeviceFacts& a, const DeviceFacts& b) {
    return a.device == b.device && a.num_cus == b.num_cus && a.scan_blocks_per_cu == b.scan_blocks_per_cu && a.pf_hw_ok == b.pf_hw_ok &&
           a.wall_khz == b.wall_khz && a.attrs16_done == b.attrs16_done;
}
static bool same(const Settings& a, const Settings& b) {
    return a.metric == b.metric && a.storage_req == b.storage_req && a.prefilter == b.prefilter && a.fused_mlp == b.fused_mlp &&
           a.stop_mass == b.stop_mass && a.path_mass == b.path_mass && a.timing_level == b.timing_level && a.chunk_rows_auto == b.chunk_rows_auto &&
           a.chunk_rows_set == b.chunk_rows_set;
}
static bool same(const Switches& a, const Switches& b) {
    return a.ps_force_wide == b.ps_force_wide && a.pf_small == b.pf_small && a.pf_redo == b.pf_redo && a.rescore_streamed == b.rescore_streamed &&
           a.pf_qbound == b.pf_qbound && a.pf_primary == b.pf_primary && a.debug_emit_all == b.debug_emit_all && a.use_tail == b.use_tail &&
           a.graded_chunks == b.graded_chunks && !memcmp(a.chunk_lvl_rows, b.chunk_lvl_rows, sizeof(a.chunk_lvl_rows)) &&
           !memcmp(a.chunk_frac, b.chunk_frac, sizeof(a.chunk_frac)) && a.use_front == b.use_front;
}

// the clone shares every model and index image as a view, and its call state is a fresh one
static void check_clone(const lmi_index* c, const lmi_index* h) {
    REQUIRE(c->parent == h && c->live_clones == 0);
    REQUIRE(same(static_cast<const DeviceFacts&>(*c), *h) && same(static_cast<const Settings&>(*c), *h) && same(static_cast<const Switches&>(*c), *h));
    REQUIRE(!memcmp(c->mut_paths, h->mut_paths, sizeof(h->mut_paths)));
    REQUIRE(c->models.size() == 3);
    for (size_t m = 0; m < 3; ++m) {
        const Model &a = c->models[m], &b = h->models[m];
        REQUIRE(a.n_layers == 2 && a.dims == b.dims && a.n_rb == b.n_rb && a.KG == b.KG && a.Wf.size() == 2 && a.bias.size() == 2);
        for (int i = 0; i < 2; ++i) REQUIRE(view_of(a.Wf[i], b.Wf[i]) && view_of(a.bias[i], b.bias[i]));
    }
    for (auto m : kModelBufs) REQUIRE(view_of(c->*m, h->*m));
    for (auto m : kImages) REQUIRE(view_of(c->*m, h->*m));
    REQUIRE(c->tree_set && !c->desc_dirty && c->fm_ok && c->fm_lds == 4096 && c->h_child_offset == h->h_child_offset &&
            c->h_child_model == h->h_child_model && c->h_child_bucket == h->h_child_bucket);
    REQUIRE(c->built && !c->building && c->N == 100 && c->d == 16 && c->L == 4 && c->KGs == 2 && c->d_user == 15 && c->chunk_rows == 512 &&
            c->n_rb_total == 5 && c->h_nb_rows == h->h_nb_rows && c->h_rb_start == h->h_rb_start && c->h_nch == h->h_nch &&
            c->h_cap_rb == h->h_cap_rb && c->h_any == h->h_any && c->h_owned.empty() && c->have16 && c->KG16 == 1 && c->dp == 16 &&
            c->storage == 1 && c->rows_added == 100 && c->owned_total == 100 && c->index_bytes() == h->index_bytes());
}
static void check_fresh_call_state(const lmi_index* c) {
    for (auto m : kWork) REQUIRE(empty(c->*m));
    REQUIRE(empty(c->act[0]) && empty(c->act[1]));
    // ... and whichever buffer the list above does not name: no word of the call state is the address of a live allocation
    const CallState& cs = *c;
    const unsigned char* bytes = reinterpret_cast<const unsigned char*>(&cs);
    for (size_t off = 0; off + sizeof(void*) <= sizeof(CallState); off += alignof(void*)) {
        void* word;
        memcpy(&word, bytes + off, sizeof(word));
        if (word == static_cast<const void*>(c->parent)) continue;   // (no allocation of hipMalloc's anyway)
        REQUIRE(!g_live.count(word));
    }
    for (int i = 0; i < 4; ++i) REQUIRE(c->h_stats[i] == 0);
    REQUIRE(!c->q_srch_async && !c->fr_bump_pending && !c->stats_pending && c->x_cap == 0 && c->overflow_armed == 0 && c->stamps_off == 0);
    REQUIRE(c->last_nslots == 0 && c->last_nb == 0 && c->last_ncols == 0 && !c->last_fast && c->ev_cur == 0 && c->ev_calls == 0);
    for (int i = 0; i < CallState::PLAN_WORDS; ++i) REQUIRE(c->last_plan[i] == 0);
    REQUIRE(c->ev == c->ev_ring[0] && c->ev_valid == c->valid_ring[0] && !c->valid_ring[5][0] && c->ts_mask[5] == 0u && !c->ts_set && !c->h_oflag);
    REQUIRE(!c->stream && !c->side && !c->side_fork && !c->side_join);
}

static void handle_rules() {
    static_assert(!std::is_copy_constructible<lmi_index>::value && !std::is_copy_assignable<lmi_index>::value,
                  "a handle is never copied whole: its call state is its own");
    for (int own_work = 0; own_work < 2; ++own_work) {
        lmi_index* h = make_parent();
        const std::set<void*> parents = g_live;
        REQUIRE(parents.size() == 3 * 4 + 4 + 12 + 14 + 2);
        {   // lmi_nav_set_model grows `models`: the models move, their weights stay where and whose they were
            static_assert(std::is_nothrow_move_constructible<Model>::value, "vector<Model> must move on growth");
            void* const w = h->models[2].Wf[1].p;
            h->models.resize(40);
            REQUIRE(h->models[2].Wf[1].p == w && !h->models[2].Wf[1].borrowed && g_live == parents);
            h->models.resize(3);
        }
        lmi_index* c = clone_handle(h);
        REQUIRE(g_live == parents && h->live_clones == 1);   // (a clone allocates nothing)
        check_clone(c, h);
        check_fresh_call_state(c);
        if (own_work) {   // the clone's own workspaces: allocations of its own, which go with it
            reserve_work(c);
            REQUIRE(g_live.size() == parents.size() + 16);
            for (auto m : kWork) REQUIRE((c->*m).p != (h->*m).p && !(c->*m).borrowed);
            REQUIRE(c->slab.reserve(c->slab.cap + 1) != 0);   // what it borrows cannot grow
            check_clone(c, h);
        }
        delete c;
        REQUIRE(g_live == parents);   // the parent's allocations are alive, the clone's own are gone
        delete h;
        REQUIRE(g_live.empty());
    }
}

int main() {
    devbuf_rules();
    handle_rules();
    REQUIRE(g_live.empty());
    printf("handle selftest: clean\n");
    return 0;
}
