// lmi_concat.h -- device side of lmi_concat (lmi_host_concat.h): a new, independent index that holds the objects of several built
// indexes over the same partition, bucket b of the result = parts[0]'s bucket b, then parts[1]'s, ...
//
// One source map (per row of the new slab: the part and the part's slab row it comes from), then one gather per stored image with the
// ids alongside, straight from the parts' slabs into the new handle's zero-filled slabs; nothing is staged.  The gathers are
// lmi_subset.h's with one more indirection: thread i fills DESTINATION piece i (a wave writes 1 KiB in address order) and the source is
// chosen per row from a small device table of the parts.  A part's rows land mid-row-block whenever the parts before it leave
// n % 32 != 0 rows in a bucket, so in the fragment forms a destination row-block may read from two or more parts: the lanes of a wave
// then differ in the part, never in the piece's place inside the row.  Every store is a plain vector store; nothing in this file is
// read by the query path.
#pragma once
#include "lmi_store16.h"
#include "lmi_subset.h"

namespace lmi {

// One part as the kernels see it.  image: the stored form's image (rowmajor / slab / slab16); maxbits, scale: LMI_STORAGE_F16 only, the
// part's xmaxbits and xscale (NULL for a part that stores no row); ratio: s_out / s_part, written by concat_scale16_kernel.
struct ConcatPart {
    const void* image;
    const uint32_t* ids;
    const unsigned* maxbits;
    const float* scale;
    float ratio;
    int pad;
};

// srcmap[new slab row] <- (part, the part's slab row), or (-1, -1) behind a bucket's last row in its last row-block.  first_row /
// n_rows / offset: [n_parts][L] -- the part's rb_start[b] * 32 and nb_rows[b] (within a part a bucket's rows are contiguous from
// there) and the plan's first in-bucket row (lmi_concat_plan.h).  grid (x, L), bucket = blockIdx.y.
__global__ void concat_srcmap_kernel(const int* __restrict__ first_row, const int* __restrict__ n_rows, const int* __restrict__ offset, int n_parts,
                                     int L, const int* __restrict__ new_rb_start, const int* __restrict__ new_nb_rows, int2* __restrict__ srcmap) {
    const int b = blockIdx.y;
    const size_t nb = (size_t)new_rb_start[b] * 32;
    const int cap = (new_rb_start[b + 1] - new_rb_start[b]) * 32, tid = blockIdx.x * blockDim.x + threadIdx.x, step = gridDim.x * blockDim.x;
    for (int t = 0; t < n_parts; ++t) {
        const int n_t = n_rows[t * L + b], src = first_row[t * L + b];
        int2* dst = srcmap + nb + offset[t * L + b];
        for (int j = tid; j < n_t; j += step) dst[j] = make_int2(t, src + j);
    }
    for (int j = new_nb_rows[b] + tid; j < cap; j += step) srcmap[nb + j] = make_int2(-1, -1);
}

// Row-major f32: subset_gather_rows_kernel with the source chosen per row.
__global__ void concat_gather_rows_kernel(const ConcatPart* __restrict__ parts, const int2* __restrict__ srcmap, long long n_rows, int per_row,
                                          float4* __restrict__ dst, uint32_t* __restrict__ dst_ids) {
    const long long total = n_rows * per_row, stride = (long long)gridDim.x * blockDim.x;
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    long long p = i / per_row;   // (row, piece) of i, carried along: one 64-bit division per thread, not one per piece
    int c = (int)(i - p * per_row);
    const long long dp = stride / per_row;
    const int dc = (int)(stride - dp * per_row);
    for (; i < total; i += stride, p += dp, c += dc) {
        if (c >= per_row) { c -= per_row; ++p; }
        const int2 s = srcmap[p];
        if (s.x < 0) continue;   // (the destination is zero-filled)
        dst[i] = static_cast<const float4*>(parts[s.x].image)[(size_t)s.y * per_row + c];
        if (c == 0) dst_ids[p] = parts[s.x].ids[s.y];
    }
}

// f32 fragments: subset_gather_frag32_kernel with the source chosen per row (the same k-group, the same half at the source row).
__global__ void concat_gather_frag32_kernel(const ConcatPart* __restrict__ parts, const int2* __restrict__ srcmap, long long n_rb, int KG,
                                            float4* __restrict__ dst, uint32_t* __restrict__ dst_ids) {
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
        const int2 s = srcmap[p];
        if (s.x < 0) continue;
        dst[i] = static_cast<const float4*>(parts[s.x].image)[((size_t)(s.y >> 5) * KG + g) * 64 + (s.y & 31) + (lane & 32)];
        if (g == 0 && lane < 32) dst_ids[p] = parts[s.x].ids[s.y];
    }
}

// The result's scale and every part's ratio (one thread).  A part stores x * s_t with s_t = scale_of_max(its max |x|, which it keeps in
// maxbits[0]); the result's maximum is the largest of the parts', so s_out <= s_t and ratio = s_out / s_t is a power of two <= 1.
// state: the new handle's xmaxbits ([0] <- the maximum, [1] <- 0: the S16_* flags the gather raises); scale: its xscale; one[0] <- 1,
// the factor storage16_images multiplies the gathered slab by.
__global__ void concat_scale16_kernel(ConcatPart* __restrict__ parts, int n_parts, unsigned* __restrict__ state, float* __restrict__ scale,
                                      float* __restrict__ one) {
    unsigned m = 0u;
    for (int t = 0; t < n_parts; ++t)
        if (parts[t].maxbits) m = max(m, parts[t].maxbits[0]);
    state[0] = m;
    state[1] = 0u;
    const float s = scale_of_max(m);
    scale[0] = s;
    scale[1] = 1.0f / s;
    for (int t = 0; t < n_parts; ++t) parts[t].ratio = parts[t].scale ? s * parts[t].scale[1] : 1.0f;
    one[0] = 1.0f;
}

// fp16 fragments (LMI_STORAGE_F16), both shapes of convert16_one: subset_gather_frag16_kernel's decoding of destination piece i, the
// source chosen per row, and the part's ratio applied to the 8 halves of the piece on the way.  THE ARITHMETIC IS rescale16_kernel's
// (lmi_store16.h) -- widen, multiply by the power of two, narrow, compare; a half that changes when it is rounded back raises
// S16_SCALE_LOSS in state[1] -- and has to stay so: the verdict is the one a fresh build of the same rows reaches.  A ratio of 1 moves
// the bits untouched.  At most one atomic per wave.
__global__ void concat_gather_frag16_kernel(const ConcatPart* __restrict__ parts, const int2* __restrict__ srcmap, long long n_rb, int KG16,
                                            int f16x16, uint4* __restrict__ dst, uint32_t* __restrict__ dst_ids, unsigned* __restrict__ state) {
    const long long total = n_rb * KG16 * 64, stride = (long long)gridDim.x * blockDim.x;   // (a multiple of 64: the lane stays)
    unsigned flags = 0u;
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = (int)(i & 63);
    long long rb = (i >> 6) / KG16;   // (row-block, fragment of the row-block) of i, carried along: one 64-bit division per thread
    int f = (int)((i >> 6) - rb * KG16);
    const long long drb = (stride >> 6) / KG16;
    const int df = (int)((stride >> 6) - drb * KG16);
    for (; i < total; i += stride, rb += drb, f += df) {
        if (f >= KG16) { f -= KG16; ++rb; }
        int k8, r;
        if (f16x16) {   // fragment f = 2 (k8 >> 2) + (r >> 4)
            k8 = 4 * (f >> 1) + (lane >> 4);
            r = 16 * (f & 1) + (lane & 15);
        } else {        // fragment f = k8 >> 1
            k8 = 2 * f + (lane >> 5);
            r = lane & 31;
        }
        const long long p = rb * 32 + r;
        const int2 s = srcmap[p];
        if (s.x < 0) continue;
        uint4 w = static_cast<const uint4*>(parts[s.x].image)[frag16_piece(s.y, k8, KG16, f16x16)];
        const float ratio = parts[s.x].ratio;
        if (ratio != 1.0f && (w.x | w.y | w.z | w.w) != 0u) {
            half8 h = __builtin_bit_cast(half8, w);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float v = (float)h[j] * ratio;
                h[j] = (_Float16)v;
                if ((float)h[j] != v) flags |= S16_SCALE_LOSS;
            }
            w = __builtin_bit_cast(uint4, h);
        }
        dst[i] = w;
        if (k8 == 0) dst_ids[p] = parts[s.x].ids[s.y];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) flags |= __shfl_xor(flags, o);
    if ((threadIdx.x & 63) == 0 && flags) atomicOr(state + 1, flags);
}

}  // namespace lmi
