// lmi_mutate.h -- device side of the index mutation calls (lmi_buckets_insert / lmi_buckets_delete, lmi_hip.hip).
//
// The scan kernels find a bucket through rb_start[b] and nb_rows[b] only and mask rows at or past n_b, so a bucket may
// sit anywhere in the slab with spare row-blocks after its last row.  Insert scatters the new rows behind a bucket's last
// row (scatter_rows_kernel / pack_scatter_kernel with a positions array of the batch, lmi_prefilter.h / lmi_kernels.h);
// delete marks the rows that stay (mark_rows_kernel, which lmi_subset shares) and compacts the hit buckets in bucket order through
// a staging buffer.  What the prefilter derives from the rows
// (the fp16 fragments, the per-bucket norm maxima) is redone for the touched row-blocks by the range-list forms below.
// Every store here is a plain vector store; nothing in this file is read by the query path.
#pragma once
#include "lmi_prefilter.h"

namespace lmi {

// ids_slab[pos[i]] <- ids[i] (pos < 0: an object of a bucket this handle does not own)
__global__ void scatter_ids_kernel(const uint32_t* __restrict__ ids, const int* __restrict__ pos, long long n,
                                   uint32_t* __restrict__ ids_slab) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int p = pos[i];
    if (p >= 0) ids_slab[p] = ids[i];
}

// Range lists: range r = blockIdx.y.  Row ranges are [row0[r], row0[r] + nrows[r]) in slab rows; block ranges
// [rb0[r], rb0[r] + nrb[r]) in row-blocks.  The host builds them for the buckets a call touched.

// max |x| over the rows of the ranges, columns [0, d) (what absmax_kernel takes over the whole slab at build time)
__global__ void absmax_ranges_kernel(const float* __restrict__ rows, int d, int pitch, const int* __restrict__ row0,
                                     const int* __restrict__ nrows, unsigned* __restrict__ out) {
    const int r = blockIdx.y;
    const long long n = (long long)nrows[r] * d;
    const float* x = rows + (size_t)row0[r] * pitch;
    float m = 0.0f;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long row = i / d;
        m = fmaxf(m, fabsf(x[row * pitch + (i - row * d)]));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0) atomicMax(out, __float_as_uint(m));
}

// convert16_kernel over row-block ranges
__global__ void convert16_ranges_kernel(const float* __restrict__ rows, int d, int pitch, const int* __restrict__ rb0,
                                        const int* __restrict__ nrb, int KG16, const float* __restrict__ scale,
                                        uint4* __restrict__ dst, int f16x16) {
    const int r = blockIdx.y;
    const long long p0 = (long long)rb0[r] * 32;
    const long long n = (long long)nrb[r] * 32 * KG16 * 2;
    const float s = scale[0];
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (long long)gridDim.x * blockDim.x)
        convert16_one(rows, d, pitch, p0 + (idx >> 1) / KG16, (int)((idx >> 1) % KG16), (int)(idx & 1), KG16, s, dst, f16x16);
}

// bucket_norm_kernel over row ranges: atomicMax of the rows' norms into their bucket's maxima (bucket[r])
__global__ void bucket_norm_ranges_kernel(const float* __restrict__ rows, int d, int pitch, const int* __restrict__ bucket,
                                          const int* __restrict__ row0, const int* __restrict__ nrows,
                                          const float* __restrict__ scale, unsigned* __restrict__ bnorm_bits,
                                          unsigned* __restrict__ bdelta_bits) {
    const int r = blockIdx.y;
    const float s = scale[0];
    const float guard = norm_guard(d);
    float best = 0.0f, bestd = 0.0f;
    for (int row = blockIdx.x * blockDim.x + threadIdx.x; row < nrows[r]; row += gridDim.x * blockDim.x)
        row_norms(rows + ((size_t)row0[r] + row) * pitch, d, s, guard, best, bestd);
    if (best > 0.0f) atomicMax(bnorm_bits + bucket[r], __float_as_uint(best));
    if (bestd > 0.0f) atomicMax(bdelta_bits + bucket[r], __float_as_uint(bestd));
}

// the maxima of the listed buckets back to 0 (before bucket_norm_ranges_kernel recomputes them after a delete)
__global__ void reset_norms_kernel(const int* __restrict__ bucket, int n, unsigned* __restrict__ bnorm_bits,
                                   unsigned* __restrict__ bdelta_bits) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    bnorm_bits[bucket[i]] = 0u;
    bdelta_bits[bucket[i]] = 0u;
}

// ---- delete, lmi_subset ----
// keep[slab row] <- 1 if the row stays (mode LMI_SUBSET_KEEP = 0: its id is in list[0..n_list), sorted ascending and unique; mode
// LMI_SUBSET_DROP = 1: it is not), else 0; kept[b] += rows that stay.  Live rows of every bucket: grid (x, L), bucket = blockIdx.y.
__global__ void mark_rows_kernel(const uint32_t* __restrict__ ids_slab, const int* __restrict__ rb_start,
                                 const int* __restrict__ nb_rows, const uint32_t* __restrict__ list, int n_list, int mode,
                                 int* __restrict__ keep, int* __restrict__ kept) {
    const int b = blockIdx.y;
    const int n_b = nb_rows[b];
    const size_t base = (size_t)rb_start[b] * 32;
    int cnt = 0;
    for (int row = blockIdx.x * blockDim.x + threadIdx.x; row < n_b; row += gridDim.x * blockDim.x) {
        const uint32_t id = ids_slab[base + row];
        int lo = 0, hi = n_list;   // first entry >= id
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (list[mid] < id) lo = mid + 1;
            else hi = mid;
        }
        const int hit = lo < n_list && list[lo] == id;
        const int stays = mode ? !hit : hit;
        keep[base + row] = stays;
        cnt += stays;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(kept + b, cnt);
}

// Stable compaction map of the hit buckets, one 1024-thread block per bucket (blockIdx.x indexes hit[]):
// src[base + j] <- the in-bucket row of the j-th kept row, -1 for j in [kept, span[i]) (the vacated tail, zero-filled by
// the gather).  keep and src are separate arrays: nothing is moved in place.
constexpr int CM_THREADS = 1024;
__global__ __launch_bounds__(CM_THREADS) void compact_map_kernel(const int* __restrict__ hit, const int* __restrict__ span,
                                                                const int* __restrict__ rb_start, const int* __restrict__ nb_rows,
                                                                const int* __restrict__ keep, int* __restrict__ src) {
    __shared__ int sc[CM_THREADS];
    const int b = hit[blockIdx.x];
    const int n_b = nb_rows[b];
    const size_t base = (size_t)rb_start[b] * 32;
    const int t = threadIdx.x;
    int carry = 0;
    for (int r0 = 0; r0 < n_b; r0 += CM_THREADS) {
        const int row = r0 + t;
        const int f = row < n_b ? keep[base + row] : 0;
        sc[t] = f;
        __syncthreads();
        for (int o = 1; o < CM_THREADS; o <<= 1) {   // inclusive Hillis-Steele scan
            const int v = t >= o ? sc[t - o] : 0;
            __syncthreads();
            sc[t] += v;
            __syncthreads();
        }
        if (f) src[base + carry + sc[t] - 1] = row;
        carry += sc[CM_THREADS - 1];
        __syncthreads();
    }
    for (int j = carry + t; j < span[blockIdx.x]; j += CM_THREADS) src[base + j] = -1;
}

// Gather of a group of compacted buckets into staging (group entry g = blockIdx.y: bucket grp_b[g], staging rows
// [grp_off[g], grp_off[g] + grp_span[g])): row j <- the bucket's row src[j] (zeros where src[j] < 0), its id likewise.
// FRAG = false: row-major f32 rows of `pitch` floats (prefilter mode), copied as float4;
// FRAG = true: the f32 fragments of the all-f32 mode (KG groups of 8 k per row, lmi_kernels.h pack_*), unpacked to
// row-major rows of `pitch` = d floats for pack_gather_kernel to pack back.
template <bool FRAG>
__global__ void gather_compact_kernel(const float* __restrict__ rows, int pitch, int KG, const uint32_t* __restrict__ ids_slab,
                                      const int* __restrict__ grp_b, const long long* __restrict__ grp_off,
                                      const int* __restrict__ grp_span, const int* __restrict__ rb_start,
                                      const int* __restrict__ src, float* __restrict__ st_rows, uint32_t* __restrict__ st_ids) {
    const int g = blockIdx.y;
    const size_t base = (size_t)rb_start[grp_b[g]] * 32;
    const long long span = grp_span[g], off = grp_off[g];
    const int per_row = FRAG ? (pitch + 7) / 8 : pitch / 4;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < span * per_row; idx += (long long)gridDim.x * blockDim.x) {
        const long long j = idx / per_row;
        const int c = (int)(idx - j * per_row);
        const int s = src[base + j];
        if (c == 0) st_ids[off + j] = s >= 0 ? ids_slab[base + s] : 0u;
        if (!FRAG) {
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (s >= 0) v = reinterpret_cast<const float4*>(rows + (base + s) * pitch)[c];
            reinterpret_cast<float4*>(st_rows + (off + j) * pitch)[c] = v;
        } else {
            float v[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            if (s >= 0) {
                const size_t p = base + s;
                const float4* f = reinterpret_cast<const float4*>(rows) + ((p >> 5) * KG + c) * 64 + (p & 31);
                const float4 e = f[0], o = f[32];
                v[0] = e.x; v[1] = o.x; v[2] = e.y; v[3] = o.y; v[4] = e.z; v[5] = o.z; v[6] = e.w; v[7] = o.w;
            }
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (8 * c + k < pitch) st_rows[(off + j) * pitch + 8 * c + k] = v[k];
        }
    }
}

}  // namespace lmi
