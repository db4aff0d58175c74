// lmi_host_gram.h -- lmi_gram and lmi_gram_f16 (one body over the type of x): argument checks, the geometry (lmi_gram_plan.h), the
// call's device buffers, the upload in pieces, and the schedule on the NULL stream of the device: max|x| and the finite check, the
// int64 column sums and the mean, the scatter matrix by tiles and piece runs, the conversion.  lmi_gram_set_geometry,
// lmi_debug_gram_plan.  What differs between the source types beside the kernels' template argument is lmi_host_kmeans.h's:
// km_absmax, km_finite, km_max_value, km_vec.
#pragma once
#include "lmi_host.h"
#include "lmi_host_call.h"
#include "lmi_host_kmeans.h"
#include "lmi_gram.h"
#include "lmi_gram_plan.h"
#include <cmath>

static_assert(LMI_GRAM_PIECE_ROWS == lmi_gram_plan::PIECE_ROWS && LMI_GRAM_PIECE_ROWS == GRAM_PIECE, "one piece length: header, plan, kernel");
static_assert(lmi_gram_plan::PANEL_ROWS == GRAM_PANEL, "lmi_gram_plan.h restates GRAM_PANEL");

namespace {

thread_local lmi_gram_plan::Forced g_gram_forced;
thread_local int64_t g_gram_last[LMI_GRAM_PLAN_COUNT] = {};

template <class T, bool VEC>
int gram_launch(int tile_cols, dim3 grid, const T* x, long long n, int d, const float* mean, const int* tile_map, long long ppb,
                double scale, unsigned long long* Tq) {
    if (tile_cols == lmi_gram_plan::TILE_SMALL) gram_kernel<T, VEC, 1><<<grid, 256>>>(x, n, d, mean, tile_map, ppb, scale, Tq);
    else gram_kernel<T, VEC, 2><<<grid, 256>>>(x, n, d, mean, tile_map, ppb, scale, Tq);
    HIPCHK(hipGetLastError());
    return 0;
}

template <class T>
int gram_run(const char* who, int device, const T* x, int64_t n, int d, float* mean, double* gram, int on_device) {
    for (int64_t& w : g_gram_last) w = 0;
    if (!x || !mean || !gram) return fail("%s: x, mean and gram must not be NULL", who);
    if (n < 1) return fail("%s: n %lld < 1", who, (long long)n);
    if (n > (1ll << 26)) return fail("%s: n %lld exceeds 2^26 (the bound of the int64 sums)", who, (long long)n);
    if (d < 1 || d > 4096) return fail("%s: d %d outside [1,4096]", who, d);
    hipDeviceProp_t prop;
    CHK(open_device(who, device, &prop));

    const lmi_gram_plan::Plan p = lmi_gram_plan::make_plan(n, d, prop.multiProcessorCount, g_gram_forced);
    const size_t xbytes = (size_t)n * d * sizeof(T), gbytes = (size_t)d * d * 8;
    CallScratch mem(who);
    T* d_x = nullptr;
    float* d_mean = nullptr;   // the call's own: 16-byte loads of it in the kernel, whatever the caller's pointer is
    double* d_gram = nullptr;
    unsigned long long *d_S = nullptr, *d_T = nullptr;
    int* d_map = nullptr;
    unsigned* d_max = nullptr;
    if (on_device) {
        d_x = const_cast<T*>(x);
        d_gram = gram;
    } else {
        CHK(mem.alloc(&d_x, xbytes, "x"));
        CHK(mem.alloc(&d_gram, gbytes, "gram"));
        CHK(upload_pieces(d_x, x, xbytes));   // the rows go up once, in the type they came in, and stay for both passes
    }
    CHK(mem.alloc(&d_mean, (size_t)d * 4, "mean"));
    CHK(mem.alloc(&d_S, (size_t)d * 8, "column sums"));
    CHK(mem.alloc(&d_T, gbytes, "scatter sums"));
    CHK(mem.alloc(&d_map, (size_t)p.tiles * 4, "tile map"));
    CHK(mem.alloc(&d_max, 4, "max"));

    // max|x| and the non-finite check, before anything of the caller's is written
    unsigned h_max = 0;
    HIPCHK(hipMemsetAsync(d_max, 0, 4, nullptr));
    const int gs = (int)std::min<long long>(prop.multiProcessorCount * 8, cdiv((long long)n * d, 256));
    km_absmax(d_x, (long long)n * d, gs, d_max);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(&h_max, d_max, 4, hipMemcpyDeviceToHost));
    if (!km_finite(d_x, h_max)) return fail("%s: x holds a value that is not finite (inf or NaN)", who);
    int e = 0;   // the smallest integer with max|x| < 2^e (0 for all-zero data)
    if (h_max) (void)std::frexp(km_max_value(d_x, h_max), &e);
    if (e > 56) return fail("%s: max|x| >= 2^56 (a piece's chain could overflow binary32)", who);

    std::vector<int> h_map((size_t)p.tiles);
    for (int64_t i = 0; i < p.tiles; ++i) {
        int ta, tb;
        lmi_gram_plan::tile_pair(p.tiles_side, i, &ta, &tb);
        h_map[(size_t)i] = ta << 16 | tb;
    }
    HIPCHK(hipMemcpy(d_map, h_map.data(), h_map.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemsetAsync(d_S, 0, (size_t)d * 8, nullptr));
    HIPCHK(hipMemsetAsync(d_T, 0, gbytes, nullptr));
    gram_sum_kernel<T><<<dim3(cdiv(n, GRAM_SUM_ROWS), cdiv(d, 64)), 256>>>(d_x, n, d, std::ldexp(1.0, 36 - e), d_S);
    gram_mean_kernel<<<cdiv(d, 256), 256>>>(reinterpret_cast<const long long*>(d_S), n, d, std::ldexp(1.0, e - 36), d_mean);
    HIPCHK(hipGetLastError());
    const bool vec = km_vec(d_x, d);
    const dim3 grid((unsigned)p.tiles, (unsigned)p.runs);
    const double scale = std::ldexp(1.0, 32 - 2 * e);
    if (vec) CHK((gram_launch<T, true>(p.tile_cols, grid, d_x, n, d, d_mean, d_map, p.pieces_per_block, scale, d_T)));
    else CHK((gram_launch<T, false>(p.tile_cols, grid, d_x, n, d, d_mean, d_map, p.pieces_per_block, scale, d_T)));
    gram_finish_kernel<<<cdiv((long long)d * d, 256), 256>>>(reinterpret_cast<const long long*>(d_T), d, std::ldexp(1.0, 2 * e - 32), d_gram);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(mean, d_mean, (size_t)d * 4, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
    if (!on_device) HIPCHK(hipMemcpy(gram, d_gram, gbytes, hipMemcpyDeviceToHost));
    HIPCHK(hipStreamSynchronize(nullptr));
    g_gram_last[LMI_GRAM_PLAN_TILE_COLS] = p.tile_cols;
    g_gram_last[LMI_GRAM_PLAN_TILES] = p.tiles;
    g_gram_last[LMI_GRAM_PLAN_PIECES] = p.pieces;
    g_gram_last[LMI_GRAM_PLAN_PIECES_PER_BLOCK] = p.pieces_per_block;
    g_gram_last[LMI_GRAM_PLAN_RUNS] = p.runs;
    g_gram_last[LMI_GRAM_PLAN_VEC] = vec;
    g_gram_last[LMI_GRAM_PLAN_EXPONENT] = e;
    g_gram_last[LMI_GRAM_PLAN_WORKSPACE_BYTES] = mem.total;
    return 0;
}

}  // namespace

extern "C" LMI_API int lmi_gram_set_geometry(int tile_cols, int64_t pieces_per_block) {
    if (tile_cols != 0 && tile_cols != lmi_gram_plan::TILE_SMALL && tile_cols != lmi_gram_plan::TILE_LARGE)
        return fail("lmi_gram_set_geometry: tile_cols %d is none of 0, %d, %d", tile_cols, lmi_gram_plan::TILE_SMALL, lmi_gram_plan::TILE_LARGE);
    if (pieces_per_block < 0 || pieces_per_block > (1ll << 14))
        return fail("lmi_gram_set_geometry: pieces_per_block %lld outside [0, 2^14]", (long long)pieces_per_block);
    g_gram_forced.tile_cols = tile_cols;
    g_gram_forced.pieces_per_block = pieces_per_block;
    return 0;
}

extern "C" LMI_API int lmi_debug_gram_plan(int64_t* out, int n) {
    if (!out || n < 0) return fail("lmi_debug_gram_plan: NULL argument");
    for (int i = 0; i < std::min(n, (int)LMI_GRAM_PLAN_COUNT); ++i) out[i] = g_gram_last[i];
    return 0;
}

extern "C" LMI_API int lmi_gram(int device, const float* x, int64_t n, int d, float* mean, double* gram, int on_device) {
    return gram_run<float>("lmi_gram", device, x, n, d, mean, gram, on_device);
}

extern "C" LMI_API int lmi_gram_f16(int device, const uint16_t* x, int64_t n, int d, float* mean, double* gram, int on_device) {
    return gram_run<uint16_t>("lmi_gram_f16", device, x, n, d, mean, gram, on_device);
}
