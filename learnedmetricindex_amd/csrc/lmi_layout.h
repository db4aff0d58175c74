// lmi_layout.h -- the arithmetic of the bucket layout: the chunk length, a fresh build's layout, the tables derived from the per-bucket
// counts, where an insert puts a bucket that outgrows its row-blocks (and when everything is re-packed instead), how a delete groups
// its buckets for staging.  Host only and pure: the standard library, no HIP call, no kernel header, no handle -- the callers
// (lmi_host_build.h, lmi_host_mutate.h) pass the tables in and act on what comes back; tests/host/layout_selftest.cpp checks it on the CPU.
//
// A bucket's rows live in row-blocks of 32; bucket b holds nb_rows[b] rows from row-block rb_start[b] on and has cap_rb[b] row-blocks
// reserved there.  A scan takes a bucket in chunks of chunk_rows rows (a multiple of TILE_ROWS), at most MAX_CHUNKS of them.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace lmi_layout {

constexpr int TILE_ROWS = 256;     // pass 2's tile (P2_TILE_ROWS, lmi_pass2.h; lmi_host.h asserts that they agree)
constexpr int MAX_CHUNKS = 1024;   // chunks a bucket is scanned in, at most

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline int64_t rup(int64_t a, int64_t b) { return cdiv(a, b) * b; }

// the last row-block a layout of L buckets may end at: slab positions are 32-bit, with 64 rows per bucket to spare (lmi_buckets_begin's limit on N)
inline int64_t max_slab_rb(int L) { return ((1ll << 31) - 64ll * L) / 32 - 1; }

// ---- chunk_rows ----
// Not set by the caller: small indexes (or small shards) get smaller chunks so that a scan has many more work items than the 256 blocks
// that share them (100 000 rows x 1 000 queries: pass 2 0.169 ms with 2048-row chunks, 0.089 ms with 256; the 1.25M-row shard of an
// 8-way split that holds the largest bucket: 0.90 ms with 2048, 0.69 ms with 512); 10M rows keep 2048.
inline int auto_chunk_rows(int64_t owned_rows, int d, bool low_d, bool prefilter) {
    int64_t c = std::min<int64_t>(2048, std::max<int64_t>(TILE_ROWS, rup(owned_rows / 4096, TILE_ROWS)));
    // d <= 128 (lmi_pass2_small.h): a 2048-row item is ~5 us of work there, about what taking it from the queue and staging its query
    // fragments costs, while 8192-row items are too few to share out evenly (10M x 45, pass 2 at 1024 / 2048 / 4096 / 8192 rows per
    // item: 0.590 / 0.441 / 0.385 / 0.412 ms): up to 4096
    if (low_d) c = std::min<int64_t>(4096, std::max<int64_t>(TILE_ROWS, rup(owned_rows / 1024, TILE_ROWS)));
    // all-f32 scan (scan_kernel: 128-query tiles, so a bucket's chunk is read by several items): the chunk's 4 d-byte rows should stay
    // in an XCD's 4-MiB L2 until the bucket's last query tile has come by -- 10M x 768: 2 048-row chunks (6 MB) 35.28 ms, 1 024-row
    // chunks 34.76 (profiles/r05_exact_chunks.txt)
    if (!prefilter) c = std::max<int64_t>(TILE_ROWS, std::min<int64_t>(c, (3ll << 20) / (4ll * d) / TILE_ROWS * TILE_ROWS));
    return (int)c;
}
// a bucket is scanned in at most MAX_CHUNKS chunks: very large buckets get larger chunks than the pick (or the caller's value)
inline int floor_chunk_rows(int chunk_rows, int max_rows) { return std::max(chunk_rows, (int)rup(cdiv(max_rows, MAX_CHUNKS), 256)); }

// ---- what follows from the per-bucket counts ----
struct AutoChunk { int d; bool low_d, prefilter; };   // auto_chunk_rows' other arguments
struct Tables {
    int64_t owned_total = 0;   // rows this handle stores
    int n_nonempty = 1;        // buckets with rows on any rank (at least 1: the queries of a batch spread over all of them, whoever owns them)
    int chunk_rows = 0;        // the pick, or the value passed in, raised to the floor
};
// nb_rows[L]: the rows stored per bucket; any[L]: the bucket holds rows on some rank (a stored row counts too); chunk_rows: the current
// value, replaced by the automatic pick where `pick` is given (a build; a mutation keeps what the build chose); nch[L] <- chunks per bucket
inline Tables derive_tables(const std::vector<int>& nb_rows, const std::vector<unsigned char>& any, int chunk_rows, const AutoChunk* pick,
                            std::vector<int>& nch) {
    const int L = (int)nb_rows.size();
    Tables t;
    int max_rows = 0, nonempty = 0;
    for (int b = 0; b < L; ++b) {
        max_rows = std::max(max_rows, nb_rows[b]);
        t.owned_total += nb_rows[b];
        nonempty += any[b] || nb_rows[b] > 0;
    }
    t.n_nonempty = std::max(1, nonempty);
    if (pick) chunk_rows = auto_chunk_rows(t.owned_total, pick->d, pick->low_d, pick->prefilter);
    t.chunk_rows = floor_chunk_rows(chunk_rows, max_rows);
    const int chunk_rb = t.chunk_rows / 32;
    nch.resize(L);
    for (int b = 0; b < L; ++b) nch[b] = (int)cdiv(cdiv(nb_rows[b], 32), chunk_rb);
    return t;
}

// A fresh build's layout: the buckets one behind the other, cdiv(n_b, 32) row-blocks each and no slack.  rb_start[L + 1], cap_rb[L];
// returns the row-blocks the layout spans (= rb_start[L]).
inline int64_t fresh_layout(const std::vector<int>& nb_rows, std::vector<int>& rb_start, std::vector<int>& cap_rb) {
    const int L = (int)nb_rows.size();
    rb_start.assign(L + 1, 0);
    cap_rb.assign(L, 0);
    for (int b = 0; b < L; ++b) {
        cap_rb[b] = (int)cdiv(nb_rows[b], 32);
        rb_start[b + 1] = rb_start[b] + cap_rb[b];
    }
    return rb_start[L];
}

// ---- insert ----
// The layout after add[b] more rows per bucket.  A bucket that outgrows its row-blocks moves behind the last row-block with geometric
// slack (its old place becomes a hole); when the tail would pass the allocations (alloc_rb row-blocks), or the holes a quarter of the
// slab, every bucket is re-packed into new allocations of alloc_new row-blocks instead.  paths: what lmi_debug_layout counts -- buckets
// that took rows in their slack, buckets relocated, growth re-packs, hole re-packs.
struct InsertPlan {
    enum Refusal { OK = 0, BUCKET_PAST_LIMIT, TOTAL_PAST_LIMIT };
    Refusal refusal = OK;
    int bucket = -1;                   // BUCKET_PAST_LIMIT: which one
    std::vector<int> start, cap;       // per bucket: first row-block, row-blocks reserved
    std::vector<unsigned char> moved;  // per bucket: it outgrew its row-blocks (without `pack`: relocated behind the old tail)
    bool pack = false;
    int64_t total = 0;                 // row-blocks the layout spans (the new n_rb_total)
    int64_t alloc_new = 0;             // row-blocks the allocations hold afterwards (pack: the new ones')
    int64_t paths[4] = {0, 0, 0, 0};
};
inline InsertPlan plan_insert(const std::vector<int>& nb_rows, const std::vector<int>& rb_start, const std::vector<int>& cap_rb,
                              int64_t n_rb_total, const std::vector<int64_t>& add, int chunk_rb, int64_t alloc_rb, int64_t max_rb) {
    const int L = (int)nb_rows.size();
    InsertPlan p;
    p.start.assign(rb_start.begin(), rb_start.begin() + L);
    p.cap = cap_rb;
    p.moved.assign(L, 0);
    int64_t tail = n_rb_total, used = 0;
    for (int b = 0; b < L; ++b) {
        const int64_t need = ((int64_t)nb_rows[b] + add[b] + 31) / 32;
        if (need > p.cap[b]) {
            // + a quarter (not x2: the images of a 10M x 768 index are 46 GB) and at least a chunk
            const int64_t c = need + std::max<int64_t>(need / 4, chunk_rb);
            if (c > max_rb) { p.refusal = InsertPlan::BUCKET_PAST_LIMIT; p.bucket = b; return p; }
            p.cap[b] = (int)c;
            p.start[b] = (int)std::min<int64_t>(tail, INT32_MAX);
            p.moved[b] = 1;
            tail += c;
        }
        used += p.cap[b];
    }
    p.pack = tail > alloc_rb || (tail - used) * 4 > tail;   // grow, or reclaim holes past a quarter of the slab
    p.total = tail;
    p.alloc_new = alloc_rb;
    if (p.pack) {
        p.total = 0;
        for (int b = 0; b < L; ++b) { p.start[b] = (int)std::min<int64_t>(p.total, INT32_MAX); p.total += p.cap[b]; }
        p.alloc_new = std::min(p.total + p.total / 8, max_rb);
    }
    // A re-pack whose packed layout fits the allocations it replaces was forced by the holes, not by the rows: with 1/8 headroom,
    // holes never pass a quarter of the slab before the tail reaches the allocation's end
    if (p.pack) {
        p.paths[p.total > alloc_rb ? 2 : 3] = 1;
    } else {
        for (int b = 0; b < L; ++b) p.paths[p.moved[b] ? 1 : 0] += add[b] > 0;
    }
    if (p.total > max_rb) p.refusal = InsertPlan::TOTAL_PAST_LIMIT;
    return p;
}

// ---- delete ----
// The hit buckets are compacted through a staging buffer, group by group, in order.  span[i]: the rows of the i-th hit bucket's
// row-blocks; a group takes buckets while their spans fit `budget` rows (a bucket longer than the budget is a group of its own).
// Group g is the hit buckets [gfirst[g], gfirst[g + 1]); goff[i]: the i-th bucket's first row in its group's staging; stage_rows: the
// longest group.
struct DeleteGroups {
    std::vector<int> gfirst;
    std::vector<long long> goff;
    int64_t stage_rows = 0;
    int n() const { return (int)gfirst.size() - 1; }
};
inline DeleteGroups delete_groups(const std::vector<int>& span, int64_t budget) {
    DeleteGroups g;
    int64_t acc = 0;
    for (size_t i = 0; i < span.size(); ++i) {
        if (i == 0 || acc + span[i] > budget) { g.gfirst.push_back((int)i); acc = 0; }
        g.goff.push_back(acc);
        acc += span[i];
        g.stage_rows = std::max(g.stage_rows, acc);
    }
    g.gfirst.push_back((int)span.size());
    return g;
}

}  // namespace lmi_layout
