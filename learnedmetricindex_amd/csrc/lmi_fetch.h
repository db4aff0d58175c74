// lmi_fetch.h -- device side of lmi_rows_fetch (lmi_host_fetch.h): stored objects by id.
//
// No table maps an id to where it lives, and none is kept (lmi_buckets_insert / _delete could only make one stale).  A call locates
// its ids with ONE pass over ids_slab and then gathers the located rows:
//   fetch_locate_kernel   every live row of the index searches its id in the call's sorted, de-duplicated request list (mark_rows_kernel's
//                         shape and search: 4N bytes read once, log2(unique) probes of a list that stays in L2) and, on a hit, lowers
//                         the id's word of the location table to (bucket << 32) | row with one 64-bit atomicMin.  The minimum of a set
//                         does not depend on the order it is taken in: among rows that share an id the word ends at the
//                         lexicographically first (bucket, row) on any grid.  A word nobody lowered stays all ones: absent.
//   fetch_gather_kernel   one lane per (request, piece of the row): the request's location word -> the slab position -> the piece out
//                         of the stored image -> the caller's row, as floats or halves.  Consecutive lanes take consecutive pieces of
//                         one request: the row-major form reads and every form writes contiguous runs.
// Every store is a plain vector store; the atomicMin above is the only atomic.  Nothing in this file is read by the query path.
#pragma once
#include "lmi_store16.h"

namespace lmi {

constexpr unsigned long long FETCH_ABSENT = ~0ull;

// loc[u] <- min(loc[u], (bucket << 32) | row) over the live rows whose id is list[u] (list: ascending, unique; loc pre-set to all ones).
// Live rows of every bucket: grid (x, L), bucket = blockIdx.y; rows at or past nb_rows[b], spare row-blocks and holes are never visited.
__global__ void fetch_locate_kernel(const uint32_t* __restrict__ ids_slab, const int* __restrict__ rb_start, const int* __restrict__ nb_rows,
                                    const uint32_t* __restrict__ list, int n_list, unsigned long long* __restrict__ loc) {
    const int b = blockIdx.y;
    const int n_b = nb_rows[b];
    const size_t base = (size_t)rb_start[b] * 32;
    for (int row = blockIdx.x * blockDim.x + threadIdx.x; row < n_b; row += gridDim.x * blockDim.x) {
        const uint32_t id = ids_slab[base + row];
        int lo = 0, hi = n_list;   // first entry >= id
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (list[mid] < id) lo = mid + 1;
            else hi = mid;
        }
        if (lo < n_list && list[lo] == id) atomicMin(loc + lo, ((unsigned long long)(unsigned)b << 32) | (unsigned)row);
    }
}

// which image fetch_gather_kernel reads (the values of lmi_host.h's StoredForm, which the host passes on)
constexpr int FETCH_FRAG32 = 0, FETCH_ROWMAJOR = 1, FETCH_FRAG16 = 2;
// columns one lane moves: a 16-byte piece of the row-major image is 4 floats, of the fp16 fragments 8 halves; a k-group of the f32
// fragments is two 16-byte pieces that interleave (unpack_kernel), so one lane takes both: 8 floats
__host__ __device__ constexpr int fetch_piece_cols(int form) { return form == FETCH_ROWMAJOR ? 4 : 8; }

struct FetchSource {
    const void* image;    // rowmajor / slab / slab16
    const float* scale;   // FETCH_FRAG16: xscale ([1] = 1 / s)
    const int* rb_start;
    int pitch;            // FETCH_ROWMAJOR: dp (floats); FETCH_FRAG32: KGs; FETCH_FRAG16: KG16
    int f16x16;           // FETCH_FRAG16: the fragment shape
    int d;                // the caller's columns (d_user)
};

// Requests [i0, i0 + n) of the call.  map[i]: the request's word of loc.  rows (nullable): [n][d] floats (HALF: halves) of THIS
// piece; bucket / row (nullable): [n] of this piece.  An absent request gets zeros and (-1, -1).  Nothing past column d is written;
// the row-major form reads nothing past the row's pitch, the fragment forms nothing past the padded K.  vec: d is a multiple of the
// piece's columns and `rows` is 16-byte aligned, so a piece is stored whole.  HALF on the two f32 forms: flag[0] <- 1 where a value
// is not finite or not binary16-exact (narrow16_kernel's rule; every writer stores the same word).
template <int FORM, bool HALF>
__global__ void fetch_gather_kernel(FetchSource S, const unsigned long long* __restrict__ loc, const int* __restrict__ map, long long i0,
                                    long long n, void* __restrict__ rows, int* __restrict__ bucket, int* __restrict__ row, int vec,
                                    unsigned* __restrict__ flag) {
    constexpr int NC = fetch_piece_cols(FORM);
    const int d = S.d;
    const int per_row = rows ? (d + NC - 1) / NC : 1;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * per_row) return;
    const long long i = idx / per_row;
    const int c = (int)(idx - i * per_row);
    const unsigned long long w = loc[map[i0 + i]];
    const bool found = w != FETCH_ABSENT;
    const int b = found ? (int)(w >> 32) : -1, r = found ? (int)(w & 0xffffffffu) : -1;
    if (c == 0) {
        if (bucket) bucket[i] = b;
        if (row) row[i] = r;
    }
    if (!rows) return;
    float v[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) v[j] = 0.0f;
    const int k0 = c * NC;
    if (found) {
        const long long p = (long long)S.rb_start[b] * 32 + r;
        if constexpr (FORM == FETCH_ROWMAJOR) {
            const float* src = static_cast<const float*>(S.image) + (size_t)p * S.pitch + k0;
            if ((S.pitch & 3) == 0) {   // 16-byte rows: the piece [k0, k0 + 4) lies inside the pitch
                const float4 x = *reinterpret_cast<const float4*>(src);
                v[0] = x.x, v[1] = x.y, v[2] = x.z, v[3] = x.w;
            } else {   // a guard, not a path that runs today: every build makes the pitch a multiple of 4 (lmi_host_build.h), so no test reaches it
#pragma unroll
                for (int j = 0; j < NC; ++j)
                    if (k0 + j < d) v[j] = src[j];
            }
        } else if constexpr (FORM == FETCH_FRAG32) {
            const float4* f = static_cast<const float4*>(S.image) + ((size_t)(p >> 5) * S.pitch + c) * 64 + (p & 31);
            const float4 e = f[0], o = f[32];
            v[0] = e.x, v[1] = o.x, v[2] = e.y, v[3] = o.y, v[4] = e.z, v[5] = o.z, v[6] = e.w, v[7] = o.w;
        } else {
            const float inv = S.scale[1];
            const half8 h = __builtin_bit_cast(half8, static_cast<const uint4*>(S.image)[frag16_piece(p, c, S.pitch, S.f16x16)]);
#pragma unroll
            for (int j = 0; j < NC; ++j) v[j] = (float)h[j] * inv;
        }
    }
    const size_t at = (size_t)i * d + k0;
    if constexpr (HALF) {
        unsigned short hv[NC];
        unsigned bad = 0u;
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            const _Float16 hx = (_Float16)v[j];
            if (FORM != FETCH_FRAG16 && k0 + j < d && (!(fabsf(v[j]) < INFINITY) || (float)hx != v[j])) bad = 1u;
            hv[j] = __builtin_bit_cast(unsigned short, hx);
        }
        if (bad) flag[0] = 1u;
        unsigned short* dst = static_cast<unsigned short*>(rows) + at;
        if (vec) {
            if constexpr (NC == 8) *reinterpret_cast<uint4*>(dst) = make_uint4(hv[0] | (unsigned)hv[1] << 16, hv[2] | (unsigned)hv[3] << 16,
                                                                                hv[4] | (unsigned)hv[5] << 16, hv[6] | (unsigned)hv[7] << 16);
            else *reinterpret_cast<uint2*>(dst) = make_uint2(hv[0] | (unsigned)hv[1] << 16, hv[2] | (unsigned)hv[3] << 16);
        } else {
#pragma unroll
            for (int j = 0; j < NC; ++j)
                if (k0 + j < d) dst[j] = hv[j];
        }
    } else {
        float* dst = static_cast<float*>(rows) + at;
        if (vec) {
            *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
            if constexpr (NC == 8) *reinterpret_cast<float4*>(dst + 4) = make_float4(v[4], v[5], v[6], v[7]);
        } else {
#pragma unroll
            for (int j = 0; j < NC; ++j)
                if (k0 + j < d) dst[j] = v[j];
        }
    }
}

}  // namespace lmi
