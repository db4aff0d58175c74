// lmi_subset.h -- device side of lmi_subset (lmi_host_subset.h): a second, independent index that holds some of a built index's objects.
//
// The rows are marked by lmi_mutate.h's mark_rows_kernel.
// The rows of the kept objects go STRAIGHT from the source handle's slabs into the new handle's zero-filled slabs, one gather per
// stored image (row-major f32, f32 fragments, fp16 fragments) with the ids alongside; nothing is staged.  The new layout is a fresh
// build's (bucket b at row-block rb_start[b], cdiv(n_b, 32) row-blocks, no slack), so the new slab never holds more rows than the old.
//
// Thread mapping of every gather: thread i moves the 16-byte piece that lands at DESTINATION piece i, so a wave writes 1 KiB in
// address order (lane l at base + 16 l); in both fp16 fragment shapes and in the f32 fragments a row-block's 32 rows of one piece are
// adjacent lanes.  What is irregular stays on the read side: a stable compaction keeps kept rows in order, so the rows a wave reads
// are ascending and, where few rows are dropped, mostly adjacent too.  Every store is a plain vector store; nothing in this file is
// read by the query path.
#pragma once
#include "lmi_mutate.h"

namespace lmi {

// srcpos[new slab row] <- the old slab row it is gathered from.  map: compact_map_kernel's output in the OLD layout (map[old base + j] =
// in-bucket row of bucket b's j-th kept row); the caller has filled srcpos with -1 (the rows behind a bucket's last in its last row-block).
// grid (x, L), bucket = blockIdx.y.
__global__ void subset_srcpos_kernel(const int* __restrict__ old_rb_start, const int* __restrict__ map, const int* __restrict__ new_rb_start,
                                     const int* __restrict__ new_nb_rows, int* __restrict__ srcpos) {
    const int b = blockIdx.y;
    const int n_b = new_nb_rows[b];
    const size_t ob = (size_t)old_rb_start[b] * 32, nb = (size_t)new_rb_start[b] * 32;
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < n_b; j += gridDim.x * blockDim.x) srcpos[nb + j] = (int)(ob + map[ob + j]);
}

// Row-major f32 (prefilter on, LMI_STORAGE_F32): row to row, `per_row` = pitch / 4 float4s each; the row's id with its first piece.
__global__ void subset_gather_rows_kernel(const float4* __restrict__ src, const uint32_t* __restrict__ src_ids, const int* __restrict__ srcpos,
                                          long long n_rows, int per_row, float4* __restrict__ dst, uint32_t* __restrict__ dst_ids) {
    const long long total = n_rows * per_row, stride = (long long)gridDim.x * blockDim.x;
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    long long p = i / per_row;   // (row, piece) of i, carried along: one 64-bit division per thread, not one per piece
    int c = (int)(i - p * per_row);
    const long long dp = stride / per_row;
    const int dc = (int)(stride - dp * per_row);
    for (; i < total; i += stride, p += dp, c += dc) {
        if (c >= per_row) { c -= per_row; ++p; }
        const int s = srcpos[p];
        if (s < 0) continue;   // (the destination is zero-filled)
        dst[i] = src[(size_t)s * per_row + c];
        if (c == 0) dst_ids[p] = src_ids[s];
    }
}

// f32 fragments (lmi_set_prefilter(0); pack_scatter_kernel's layout: k-group g of slab row p is the float4s e, o at
// ((p >> 5) * KG + g) * 64 + (p & 31) + {0, 32}).  Destination piece i = ((rb * KG + g) * 64 + lane): row 32 rb + (lane & 31), e or o by
// lane >> 5 -- the same g, the same half at the source row.
__global__ void subset_gather_frag32_kernel(const float4* __restrict__ src, const uint32_t* __restrict__ src_ids, const int* __restrict__ srcpos,
                                            long long n_rb, int KG, float4* __restrict__ dst, uint32_t* __restrict__ dst_ids) {
    const long long total = n_rb * KG * 64, stride = (long long)gridDim.x * blockDim.x;   // (a multiple of 64: the lane stays)
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = (int)(i & 63);
    long long rb = (i >> 6) / KG;   // (row-block, k-group) of i, carried along: one 64-bit division per thread
    int g = (int)((i >> 6) - rb * KG);
    const long long drb = (stride >> 6) / KG;
    const int dg = (int)((stride >> 6) - drb * KG);
    for (; i < total; i += stride, rb += drb, g += dg) {
        if (g >= KG) { g -= KG; ++rb; }
        const long long p = rb * 32 + (lane & 31);
        const int s = srcpos[p];
        if (s < 0) continue;
        dst[i] = src[((size_t)(s >> 5) * KG + g) * 64 + (s & 31) + (lane & 32)];
        if (g == 0 && lane < 32) dst_ids[p] = src_ids[s];
    }
}

// fp16 fragments (LMI_STORAGE_F16), both shapes of convert16_one: destination piece i is decoded to (slab row p, k8) -- the inverse of
// frag16_piece -- and filled from frag16_piece(source row, k8).  The same pass takes the kept rows' max |half| (maxbits[0], the bits of
// the binary32 value: a non-negative half's bit pattern orders like its value, so the maximum is taken on the patterns).
__global__ void subset_gather_frag16_kernel(const uint4* __restrict__ src, const uint32_t* __restrict__ src_ids, const int* __restrict__ srcpos,
                                            long long n_rb, int KG16, int f16x16, uint4* __restrict__ dst, uint32_t* __restrict__ dst_ids,
                                            unsigned* __restrict__ maxbits) {
    const long long total = n_rb * KG16 * 64, stride = (long long)gridDim.x * blockDim.x;   // (a multiple of 64: the lane stays)
    unsigned m = 0u;
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = (int)(i & 63);
    long long rb = (i >> 6) / KG16;   // (row-block, fragment of the row-block) of i, carried along: one 64-bit division per thread
    int f = (int)((i >> 6) - rb * KG16);
    const long long drb = (stride >> 6) / KG16;
    const int df = (int)((stride >> 6) - drb * KG16);
    for (; i < total; i += stride, rb += drb, f += df) {
        if (f >= KG16) { f -= KG16; ++rb; }
        int k8, r;
        if (f16x16) {   // (((rb * (KG16 / 2) + (k8 >> 2)) * 2 + (r >> 4)) * 64 + 16 (k8 & 3) + (r & 15): fragment f = 2 (k8 >> 2) + (r >> 4)
            k8 = 4 * (f >> 1) + (lane >> 4);
            r = 16 * (f & 1) + (lane & 15);
        } else {        // (rb * KG16 + (k8 >> 1)) * 64 + 32 (k8 & 1) + r: fragment f = k8 >> 1
            k8 = 2 * f + (lane >> 5);
            r = lane & 31;
        }
        const long long p = rb * 32 + r;
        const int s = srcpos[p];
        if (s < 0) continue;
        const uint4 w = src[frag16_piece(s, k8, KG16, f16x16)];
        dst[i] = w;
        if (k8 == 0) dst_ids[p] = src_ids[s];
        const unsigned a = w.x & 0x7FFF7FFFu, b = w.y & 0x7FFF7FFFu, c = w.z & 0x7FFF7FFFu, e = w.w & 0x7FFF7FFFu;
        m = max(max(max(a & 0xFFFFu, a >> 16), max(b & 0xFFFFu, b >> 16)), max(m, max(max(c & 0xFFFFu, c >> 16), max(e & 0xFFFFu, e >> 16))));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
    if ((threadIdx.x & 63) == 0 && m) atomicMax(maxbits, __float_as_uint((float)__builtin_bit_cast(_Float16, (unsigned short)m)));
}

// The scale of the new LMI_STORAGE_F16 index from the kept rows' maximum.  The stored halves are x * s_old, so max |half| / s_old is the
// kept rows' max |x| (exact: a power of two) -- what the ingest of a fresh build leaves in state[0]; scale_of_max gives s_new >= s_old
// from it as make_scale_kernel does, and ratio[0] = s_new / s_old is the power of two rescale16_kernel multiplies the pieces by.
__global__ void subset_scale16_kernel(const unsigned* __restrict__ maxbits, const float* __restrict__ old_scale, unsigned* __restrict__ state,
                                      float* __restrict__ scale, float* __restrict__ ratio) {
    const float m = __uint_as_float(maxbits[0]) * old_scale[1];
    state[0] = __float_as_uint(m);
    state[1] = 0u;
    const float s = scale_of_max(state[0]);
    scale[0] = s;
    scale[1] = 1.0f / s;
    ratio[0] = s * old_scale[1];
}

}  // namespace lmi
