// lmi_union.h -- device code of the union scan (lmi_scan_union, lmi_search_union, lmi_search_tree_union): for every query the k best
// objects of the union of its visited buckets, k up to 1024 (include/lmi_hip.h states the contract).
//
// A slot is one (query, rank) whose bucket has rows.  The host sorts a query group's slots by bucket, cuts them into waves and writes
// the tables the kernels below are launched from (lmi_union_plan.h, build_tables; lmi_host_union.h uploads them and launches); per wave:
//   union_pack_kernel    the wave's slot queries, gathered by an index list, into fragment order (dense_pack_kernel with the list);
//   union_score_kernel   one block per item = (bucket, 256 rows of it, CT query tiles): S = Q . X^T by v_mfma_f32_32x32x2_f32,
//                        knn_score_kernel's loop (the two and km_assign_kernel are kept equal: lmi_dense.h) with B straight from the
//                        row-major image (dense_load_b on pitch dp, width d, tail 0: for L2 the stored -|x|^2/2 column meets the 1 of
//                        the augmented query inside the chain).  A slot's scores are one row of the wave's slab;
//   union_select_kernel  one wave per slot: knn_select_wave over the slot's slab row into the slot's OWN list, entries
//                        (score bits, ordinal) -- no two slots share a list, so nothing is written concurrently.
// Per group, union_finish_kernel merges a query's nb lists (knn_merge_kernel's scheme), maps each ordinal to (rank, row), the row to
// its slab position and id, the score to the scan's dist, and writes padding and counts.  union_finish_part_kernel is the same body
// writing a part (lmi_scan_union_part: score, dist, id, rank, row per result) for the merge across ranks (lmi_union_merge.h).
#pragma once
#include "lmi_knn.h"
#include "lmi_union_plan.h"

namespace lmi {

// UnionItem (one block of union_score_kernel) and UnionSlot (one block of union_select_kernel) are declared in lmi_union_plan.h, in
// this namespace, beside the pure host code that builds the tables of them.

// dense_pack_kernel with an index list: fragment row p holds query rowq[p] (rowq[p] < 0: zeros) of src [.][d]; links >= d: zeros.
__global__ void union_pack_kernel(const float* __restrict__ src, const int* __restrict__ rowq, int d, int nct, int KG,
                                  float4* __restrict__ dst) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)nct * 32 * KG) return;
    const int g = (int)(idx % KG);
    const int p = (int)(idx / KG);
    const int q = rowq[p];
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int t = g * 8 + j;
        v[j] = q >= 0 && t < d ? src[(size_t)q * d + t] : 0.0f;
    }
    float4* f = dst + ((size_t)(p >> 5) * KG + g) * 64 + (p & 31);
    f[0] = make_float4(v[0], v[2], v[4], v[6]);
    f[32] = make_float4(v[1], v[3], v[5], v[7]);
}

// grid = items, block 256: wave w -> rows [(it.blk * 4 + w) * 64, +64) of the bucket as KNN_XB column blocks, against the query tiles
// [it.tile0, + it.ntiles).  rows: the row-major image, pitch dp floats, d links used.  Qf [tiles][KG][64], KG a multiple of 4.
// Tile T's queries 0 .. tile_cnt[T]-1 write S[tile_off[T] + query * rup(n, 64) + row].
template <int CT, bool VEC>
__global__ __launch_bounds__(256) void union_score_kernel(const UnionItem* __restrict__ items, const float* __restrict__ rows, int dp, int d,
                                                          const float4* __restrict__ Qf, int KG, const long long* __restrict__ tile_off,
                                                          const int* __restrict__ tile_cnt, float* __restrict__ S) {
    const UnionItem it = items[blockIdx.x];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, h = lane >> 5, c = lane & 31;
    const long long n = it.n;
    const long long row0 = ((long long)it.blk * 4 + w) * (KNN_XB * 32);
    if (row0 >= n) return;
    const float* x = rows + (size_t)it.pos0 * dp;
    const float* xr[KNN_XB];
#pragma unroll
    for (int b = 0; b < KNN_XB; ++b) {
        const long long r = row0 + b * 32 + c;
        const long long rc = r < n ? r : n - 1;   // clamp: duplicates are computed and not written
        xr[b] = x + (size_t)rc * dp;
    }
    const int nch = KG >> 2;
    f32x16 acc[CT][KNN_XB];
#pragma unroll
    for (int t = 0; t < CT; ++t)
#pragma unroll
        for (int b = 0; b < KNN_XB; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][b][r] = 0.0f;
    const float4* ap[CT];
#pragma unroll
    for (int t = 0; t < CT; ++t) ap[t] = Qf + (size_t)(it.tile0 + (t < it.ntiles ? t : it.ntiles - 1)) * KG * 64 + lane;
    float bv[KNN_XB][16];
#pragma unroll
    for (int b = 0; b < KNN_XB; ++b) dense_load_b<VEC>(xr[b], d, 0, h, 0.0f, bv[b]);
    float4 a[CT];
#pragma unroll
    for (int t = 0; t < CT; ++t) a[t] = ap[t][0];
    for (int ch = 0; ch < nch; ++ch) {
        // the next chunk's rows are requested before this chunk's MFMAs (the last chunk reads itself again)
        float bn[KNN_XB][16];
        const int chn = ch + 1 < nch ? ch + 1 : ch;
#pragma unroll
        for (int b = 0; b < KNN_XB; ++b) dense_load_b<VEC>(xr[b], d, chn, h, 0.0f, bn[b]);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int gn = ch * 4 + g + 1 < KG ? ch * 4 + g + 1 : ch * 4 + g;
            float4 an[CT];
#pragma unroll
            for (int t = 0; t < CT; ++t) an[t] = ap[t][(size_t)gn * 64];
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int t = 0; t < CT; ++t) {
                    const float av = s == 0 ? a[t].x : s == 1 ? a[t].y : s == 2 ? a[t].z : a[t].w;
#pragma unroll
                    for (int b = 0; b < KNN_XB; ++b)
                        acc[t][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv[b][4 * g + s], acc[t][b], 0, 0, 0);
                }
#pragma unroll
            for (int t = 0; t < CT; ++t) a[t] = an[t];
        }
#pragma unroll
        for (int b = 0; b < KNN_XB; ++b)
#pragma unroll
            for (int s = 0; s < 16; ++s) bv[b][s] = bn[b][s];
    }
    // a lane holds one row of the bucket and 16 queries of every tile: 32 lanes write 128 consecutive bytes of a slot's slab row
    const long long pitch = (n + 63) / 64 * 64;
#pragma unroll
    for (int t = 0; t < CT; ++t) {
        if (t >= it.ntiles) continue;
        const int cnt = tile_cnt[it.tile0 + t];
        float* st = S + tile_off[it.tile0 + t];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int q = acc_row(r, h);
            if (q >= cnt) continue;
#pragma unroll
            for (int b = 0; b < KNN_XB; ++b) {
                const long long row = row0 + b * 32 + c;
                if (row < n) st[(size_t)q * pitch + row] = acc[t][b][r];
            }
        }
    }
}

// grid = the wave's slots, block 64, dynamic LDS 2 * LR entries: the slot's list <- the first k of its slab row in the total order
__global__ __launch_bounds__(64) void union_select_kernel(const float* __restrict__ S, const UnionSlot* __restrict__ slots, int k, int LR,
                                                          knn_entry* __restrict__ lists) {
    const UnionSlot sl = slots[blockIdx.x];
    knn_select_wave(S + sl.s_off, 0, sl.n, sl.base, k, LR, lists + sl.list, true);
}

// One wave, dynamic LDS 2 * LR entries.  Query q (of the group): merges the lists of its ranks with rows (slot_n[q][t] > 0; the others
// were never written) and writes D[q][k], I[q][k], counts[q] (nullable).  An entry's ordinal o belongs to the last rank t with
// slot_base[q][t] <= o (the bases are the exclusive sums of slot_n: a rank without rows shares its successor's base and is never the
// last); its object is row o - base of that bucket, at slab position slot_pos0[q][t] + row.  dist: sim_to_dist.
// PART: D and I are not used; part [LMI_UNION_PART_PLANES][plane] int32 words, plane = the words between two planes, gets at
// q * k + j the score's bits, the dist's bits, the id, the rank t and the row (behind the real results: -FLT_MAX, +inf, 0, ~0, ~0).
template <bool PART>
__device__ __forceinline__ void union_finish_body(const knn_entry* __restrict__ lists, const int* __restrict__ slot_n,
                                                  const unsigned* __restrict__ slot_base, const long long* __restrict__ slot_pos0, int nb,
                                                  int LR, int k, const float* __restrict__ qn2, const unsigned* __restrict__ ids_slab,
                                                  float* __restrict__ D, unsigned* __restrict__ I, int* __restrict__ counts,
                                                  int* __restrict__ part, long long plane) {
    extern __shared__ knn_entry knn_lds[];
    const int lane = threadIdx.x, q = blockIdx.x;
    const int* sn = slot_n + (size_t)q * nb;
    const unsigned* sb = slot_base + (size_t)q * nb;
    const long long* sp = slot_pos0 + (size_t)q * nb;
    for (int i = lane; i < LR; i += 64) knn_lds[i] = KNN_EMPTY;
    __syncthreads();
    for (int t = 0; t < nb; ++t) {
        if (sn[t] <= 0) continue;   // uniform
        const knn_entry* l = lists + ((size_t)q * nb + t) * LR;
        for (int i = lane; i < LR; i += 64) knn_lds[LR + i] = l[LR - 1 - i];
        __syncthreads();
        knn_bitonic_merge(knn_lds, 2 * LR, lane);
    }
    int real = 0;   // uniform
    for (int j0 = 0; j0 < k; j0 += 64) {
        const int j = j0 + lane;
        const knn_entry e = j < k ? knn_lds[j] : KNN_EMPTY;
        const bool have = knn_row(e) != 0xffffffffu;
        real += __popcll(__ballot(have));
        if (j >= k) continue;
        float dv = __builtin_inff();
        unsigned iv = 0u;
        [[maybe_unused]] unsigned rank = 0xffffffffu, row = 0xffffffffu;
        if (have) {
            const unsigned o = knn_row(e);
            int lo = 0, hi = nb - 1;   // the last t with sb[t] <= o
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (sb[mid] <= o) lo = mid;
                else hi = mid - 1;
            }
            iv = ids_slab[sp[lo] + (long long)(o - sb[lo])];
            dv = sim_to_dist(knn_score(e), qn2, q);
            if constexpr (PART) { rank = (unsigned)lo; row = o - sb[lo]; }
        }
        if constexpr (PART) {
            int* out = part + (size_t)q * k + j;
            out[0 * plane] = (int)(have ? (unsigned)(e >> 32) : (unsigned)(KNN_EMPTY >> 32));
            out[1 * plane] = (int)__float_as_uint(dv);
            out[2 * plane] = (int)iv;
            out[3 * plane] = (int)rank;
            out[4 * plane] = (int)row;
        } else {
            D[(size_t)q * k + j] = dv;
            I[(size_t)q * k + j] = iv;
        }
    }
    if (counts && lane == 0) counts[q] = real;
}

// grid = the group's queries, block 64, dynamic LDS 2 * LR entries
__global__ __launch_bounds__(64) void union_finish_kernel(const knn_entry* __restrict__ lists, const int* __restrict__ slot_n,
                                                          const unsigned* __restrict__ slot_base, const long long* __restrict__ slot_pos0,
                                                          int nb, int LR, int k, const float* __restrict__ qn2,
                                                          const unsigned* __restrict__ ids_slab, float* __restrict__ D,
                                                          unsigned* __restrict__ I, int* __restrict__ counts) {
    union_finish_body<false>(lists, slot_n, slot_base, slot_pos0, nb, LR, k, qn2, ids_slab, D, I, counts, nullptr, 0);
}
__global__ __launch_bounds__(64) void union_finish_part_kernel(const knn_entry* __restrict__ lists, const int* __restrict__ slot_n,
                                                               const unsigned* __restrict__ slot_base,
                                                               const long long* __restrict__ slot_pos0, int nb, int LR, int k,
                                                               const float* __restrict__ qn2, const unsigned* __restrict__ ids_slab,
                                                               int* __restrict__ part, long long plane, int* __restrict__ counts) {
    union_finish_body<true>(lists, slot_n, slot_base, slot_pos0, nb, LR, k, qn2, ids_slab, nullptr, nullptr, counts, part, plane);
}

}  // namespace lmi
